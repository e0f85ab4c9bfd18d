"""Where the gates of tests/test_gpu_f64_pgrad.py come from: the float64 CPU oracle's parameter gradients against themselves when
the summation order changes -- the only freedom a correct float64 statement has.  ``orc.function_param_vjp`` (and autograd through
a two-layer MLP) is run on every graph of the test with its edge list permuted and with its nodes renumbered (three seeds each);
printed per graph: the worst relative L2 over the matrix tensors, over the vectors / scalars, of ``J^T w`` and of ``dH_init``, and
the tensor that is worst.  CPU only:

    python scripts/calib_f64_pgrad.py
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import limit_graphs as lg   # noqa: E402
from conftest import CASES, load_case, load_weights, pkg   # noqa: E402
from oracle import psignn_oracle as orc   # noqa: E402
from test_gpu_f64 import FIXTURES, _random_two_layer_mixed   # noqa: E402
from test_gpu_plan_limits import _random_two_layer, _to64   # noqa: E402

torch.set_default_dtype(torch.float64)


def rel(a, b):
    d = float(b.norm())
    return float((a - b).norm()) / d if d > 0 else float((a - b).norm())


def permuted(mesh, H, h0, w, seed, nodes):
    """The same problem with the edge list in another order, or (nodes) with the nodes renumbered; returns the inverse map too."""
    gen = torch.Generator().manual_seed(seed)
    m = mesh.clone()
    N, E = mesh.num_nodes, mesh.edge_index.shape[1]
    if not nodes:
        pe = torch.randperm(E, generator=gen)
        for k, v in list(vars(mesh).items()):
            if torch.is_tensor(v) and v.dim() >= 1 and v.shape[0] == E and k != "edge_index" and E != N:
                setattr(m, k, v[pe])
        m.edge_index = mesh.edge_index[:, pe]
        return m, H, h0, w, None
    pn = torch.randperm(N, generator=gen)   # new row i is old row pn[i]
    inv = torch.empty_like(pn)
    inv[pn] = torch.arange(N)
    for k, v in list(vars(mesh).items()):
        if torch.is_tensor(v) and v.dim() >= 1 and v.shape[0] == N and k != "edge_index" and E != N:
            setattr(m, k, v[pn])
    m.edge_index = inv[mesh.edge_index]
    return m, H[pn], h0[pn], w[pn], inv


def spread(name, sd, mesh, H, h0, w):
    s64, m64 = _to64(sd, mesh)
    base = orc.function_param_vjp(s64, H.clone(), h0, m64, w)
    worst = {"matrix": (0.0, ""), "vector": (0.0, ""), "jtw": (0.0, ""), "init": (0.0, "")}

    def note(kind, r, what):
        if r > worst[kind][0]:
            worst[kind] = (r, what)
    for nodes in (False, True):
        for seed in (1, 2, 3):
            mp, Hp, h0p, wp, inv = permuted(m64, H, h0, w, seed, nodes)
            g, jtw, init = orc.function_param_vjp(s64, Hp.clone(), h0p, mp, wp)
            if inv is not None:
                jtw, init = jtw[inv], init[inv]
            for k, t in g.items():
                if t is None:
                    assert base[0][k] is None, k
                    continue
                note("matrix" if t.dim() == 2 and t.shape[0] > 1 else "vector", rel(t, base[0][k]), k)
            note("jtw", rel(jtw, base[1]), "J^T w")
            note("init", rel(init, base[2]), "dH_init")
    print(f"{name:34s} matrices {worst['matrix'][0]:.1e} ({worst['matrix'][1]})  vectors {worst['vector'][0]:.1e} "
          f"({worst['vector'][1]})  J^T w {worst['jtw'][0]:.1e}  dH_init {worst['init'][0]:.1e}", flush=True)
    return worst


def randn(shape, seed, scale=1.0):
    return scale * torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def main():
    for name in FIXTURES:
        g, mesh = load_case(name)
        sd = load_weights(CASES[name])
        s64, m64 = _to64(sd, mesh)
        with torch.no_grad():
            h0 = orc.encoder(s64, m64.x)
        for at, H in (("h0", h0), ("fp64_result", torch.from_numpy(g["fp64_result"]))):
            spread(f"{name} at {at}", sd, mesh, H, h0, randn(H.shape, 31))
    for case in ("slots255_split", "ragged65", "slots256"):
        for mixed in (False, True):
            c = lg.build(case, mixed)
            N = c.mesh.num_nodes
            gen = torch.Generator().manual_seed(21)
            H = 0.3 * torch.randn(N, 10, generator=gen, dtype=torch.float64)
            H0 = 0.3 * torch.randn(N, 10, generator=gen, dtype=torch.float64)
            spread(f"{case} {'mixed' if mixed else 'dirichlet'} ({N})", load_weights("mixed" if mixed else "dirichlet"), c.mesh, H, H0,
                   randn(H.shape, 31))
    for mixed in (False, True):
        _, mesh = load_case("hex13_mixed_s1" if mixed else "hex13_dirichlet_s0")
        sd = _random_two_layer_mixed() if mixed else _random_two_layer()
        gen = torch.Generator().manual_seed(22)
        H = 0.3 * torch.randn(mesh.num_nodes, 10, generator=gen, dtype=torch.float64)
        H0 = 0.3 * torch.randn(mesh.num_nodes, 10, generator=gen, dtype=torch.float64)
        spread(f"two layers {'mixed' if mixed else 'dirichlet'}", sd, mesh, H, H0, randn(H.shape, 31))
    for mixed in (False, True):
        mesh = pkg("data").make_hex_problem(60, seed=3, mixed=mixed, compute_sol=False)
        sd = load_weights("mixed" if mixed else "dirichlet")
        s64, m64 = _to64(sd, mesh)
        with torch.no_grad():
            h0 = orc.encoder(s64, m64.x)
        spread(f"hex60 {'mixed' if mixed else 'dirichlet'} dense", sd, mesh, h0, h0, randn(h0.shape, 31))
        w = torch.zeros_like(h0)
        N = mesh.num_nodes
        for c in (128,):
            rows = [0, c - 1, c, c + 1, 2 * c - 1, 2 * c, N - 1]
            w[rows] = randn((len(rows), 10), 32)
        spread(f"hex60 {'mixed' if mixed else 'dirichlet'} probe", sd, mesh, h0, h0, w)
    # the MLP backward: autograd under a permutation of the rows
    mlps = []
    for fam in ("dirichlet", "mixed"):
        sd = load_weights(fam)
        for which in ("encoder", "decoder"):
            mlps.append((f"{fam} {which}", [sd[f"autoencoder.{which}.mlp.mlp.{i}.{p}"].double()
                                            for i, p in ((0, "weight"), (0, "bias"), (2, "weight"), (2, "bias"))]))
    gen = torch.Generator().manual_seed(7)
    mlps.append(("random 16-16-16", [torch.randn(16, 16, generator=gen) * 0.3, torch.randn(16, generator=gen) * 0.1,
                                     torch.randn(16, 16, generator=gen) * 0.3, torch.randn(16, generator=gen) * 0.1]))
    for name, ws in mlps:
        for n in (1, 255, 257, 10981):
            x, gy = randn((n, ws[0].shape[1]), 41), randn((n, ws[2].shape[0]), 42)

            def grads(x, gy):
                xs = x.clone().requires_grad_(True)
                ps = [t.clone().requires_grad_(True) for t in ws]
                y = torch.nn.functional.linear(torch.relu(torch.nn.functional.linear(xs, ps[0], ps[1])), ps[2], ps[3])
                return torch.autograd.grad(y, [xs] + ps, gy)
            base = grads(x, gy)
            worst = [0.0, 0.0]
            for seed in (1, 2, 3):
                pn = torch.randperm(n, generator=torch.Generator().manual_seed(seed))
                inv = torch.empty_like(pn)
                inv[pn] = torch.arange(n)
                g = grads(x[pn], gy[pn])
                worst[0] = max(worst[0], rel(g[0][inv], base[0]))
                worst[1] = max([worst[1]] + [rel(a, b) for a, b in zip(g[1:], base[1:])])
            print(f"mlp {name:22s} n {n:6d}: gx {worst[0]:.1e}  parameters {worst[1]:.1e}", flush=True)


if __name__ == "__main__":
    main()
