"""Where the gates of tests/test_gpu_f64_vjp_backward.py come from: the float64 CPU oracle's backward of the VJP
(``orc.function_vjp_backward``) against itself when the summation order changes -- the only freedom a correct float64 statement
has.  It is run on every case of the test (tests/vjp_backward_cases.py) with its edge list permuted and with its nodes renumbered,
three seeds each; printed per case: the worst relative L2 over the matrix tensors, over the vectors / scalars, of ``dH`` and of
``J^T V``, and the tensor that is worst.  Then, on the hex60 mesh, the defect the oracle itself leaves in the exact identities of
the test (symmetry of the Hessian, linearity in Gbar).  CPU only:

    python scripts/calib_f64_vjp_backward.py
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vjp_backward_cases as vb   # noqa: E402
from oracle import psignn_oracle as orc   # noqa: E402

torch.set_default_dtype(torch.float64)


def rel(a, b):
    d = float(b.norm())
    return float((a - b).norm()) / d if d > 0 else float((a - b).norm())


def permuted(mesh, rows, seed, nodes):
    """The same problem with the edge list in another order, or (nodes) with the nodes renumbered: the mesh, the (N, 10) arrays in
    ``rows`` in its numbering, and the map back (None when the numbering is unchanged)."""
    gen = torch.Generator().manual_seed(seed)
    m = mesh.clone()
    N, E = mesh.num_nodes, mesh.edge_index.shape[1]
    if not nodes:
        pe = torch.randperm(E, generator=gen)
        for k, v in list(vars(mesh).items()):
            if torch.is_tensor(v) and v.dim() >= 1 and v.shape[0] == E and k != "edge_index" and E != N:
                setattr(m, k, v[pe])
        m.edge_index = mesh.edge_index[:, pe]
        return m, rows, None
    pn = torch.randperm(N, generator=gen)   # new row i is old row pn[i]
    inv = torch.empty_like(pn)
    inv[pn] = torch.arange(N)
    for k, v in list(vars(mesh).items()):
        if torch.is_tensor(v) and v.dim() >= 1 and v.shape[0] == N and k != "edge_index" and E != N:
            setattr(m, k, v[pn])
    m.edge_index = inv[mesh.edge_index]
    return m, [r[pn] for r in rows], inv


def spread(c):
    s64, m64 = vb.to64(c.sd, c.mesh)
    h0 = vb.encoded(c.sd, c.mesh) if c.h0 is None else c.h0
    base = orc.function_vjp_backward(s64, c.H.clone(), h0, m64, c.V, c.Gbar)
    worst = {"matrix": (0.0, ""), "vector": (0.0, ""), "dh": (0.0, ""), "jtv": (0.0, "")}

    def note(kind, r, what):
        if r > worst[kind][0]:
            worst[kind] = (r, what)
    if m64.edge_index.shape[1] == m64.num_nodes:
        print(f"{c.name:34s} one edge per node: the permutation helper cannot tell edge arrays from node arrays, not permuted")
        return worst
    for nodes in (False, True):
        for seed in (1, 2, 3):
            mp, (Hp, h0p, Vp, Gp), inv = permuted(m64, [c.H, h0, c.V, c.Gbar], seed, nodes)
            g, dh, jtv = orc.function_vjp_backward(s64, Hp.clone(), h0p, mp, Vp, Gp)
            if inv is not None:
                dh, jtv = dh[inv], jtv[inv]
            for k, t in g.items():
                note("matrix" if t.dim() == 2 and t.shape[0] > 1 else "vector", rel(t, base[0][k]), k)
            note("dh", rel(dh, base[1]), "dH")
            note("jtv", rel(jtv, base[2]), "J^T V")
    print(f"{c.name:34s} matrices {worst['matrix'][0]:.1e} ({worst['matrix'][1]})  vectors {worst['vector'][0]:.1e} "
          f"({worst['vector'][1]})  dH {worst['dh'][0]:.1e}  J^T V {worst['jtv'][0]:.1e}", flush=True)
    return worst


def main():
    tot = {"matrix": 0.0, "vector": 0.0, "dh": 0.0, "jtv": 0.0}
    for name in vb.NAMES:
        w = spread(vb.make(name))
        for k in tot:
            tot[k] = max(tot[k], w[k][0])
    print("worst over the cases: " + "  ".join(f"{k} {v:.1e}" for k, v in tot.items()), flush=True)
    for mixed in (False, True):
        c = vb.make(f"hex60-{'mixed' if mixed else 'dirichlet'}-dense")
        a, b = vb.randn(c.H.shape, 41), vb.randn(c.H.shape, 43)
        sym, lin_p, lin_h = vb.identity_defects(lambda G: vb.oracle(c, Gbar=G), a, b)
        print(f"{c.name:34s} oracle's own defect: symmetry {sym:.1e}  linearity parameters {lin_p:.1e}  dH {lin_h:.1e}", flush=True)


if __name__ == "__main__":
    main()
