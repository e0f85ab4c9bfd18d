"""GPU: the float64 twin of the forward path (``psignn_f64_*``, ``psignn_mlp2_f64``, ``psignn_broyden64_*``; ``engine.PackedWeights64``,
``mlp2_64``, ``FixedPointMap64``, ``DeviceBroyden64``, ``fixed_point64``) against the CPU oracle in float64.

The oracle sides run with ``torch.set_default_dtype(torch.float64)`` switched for the call only, as oracle/make_golden.py does (the
reference's broyden allocates its pairs in the default dtype).  Where the gates come from:

* f and the MLP (tests 1-3, 8): relative L2 <= 1e-13 and max-abs <= 1e-12.  The float64 oracle against itself with its edges
  permuted gives <= 2.6e-16 and <= 3.8e-15 on the limit graphs used here (outputs are O(3)); the gates are about 250 x that spread,
  which leaves room for the device's exp / sqrt differing by a few ulp.
* first iterations (test 4): entries 0-9 of both traces, rtol 1e-9.  A rounding-level perturbation of f (+-4 ulp per element) moves
  those entries by at most 2.5e-11 on hex13 (both families) and hex26; the first entry to move by more than 1e-10 is number 12.
  Later entries are not compared: Broyden trajectories are chaotic.
* converged (test 5): the oracle's own float64 solve under that perturbation, or from another start, ends 1.5e-10 - 5.3e-10 from the
  stored result; the gate 5e-9 is 10 x the worst.
* tight (test 6): the distance between a 1e-11 and a 1e-13 solution is 11 - 16 x the looser residual; the gate 50 x the sum of the
  two residuals leaves a margin of 3 x.
"""
import contextlib
import functools

import numpy as np
import pytest
import torch

import limit_graphs as lg
from conftest import CASES, load_case, load_weights, pkg, rel_l2
from oracle import psignn_oracle as orc
from test_gpu_plan_limits import _random_two_layer, _to64

pytestmark = pytest.mark.gpu

FIXTURES = ["hex13_dirichlet_s0", "hex13_mixed_s1", "original_dirichlet_s0"]
GATE_REL, GATE_ABS = 1e-13, 1e-12


@contextlib.contextmanager
def float64_default():
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        yield
    finally:
        torch.set_default_dtype(old)


def _close(got, want, what):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    rel, mx = rel_l2(got, want), float((got - want).abs().max())
    print(f"F64 {what}: rel L2 {rel:.2e} max-abs {mx:.2e}")
    assert rel <= GATE_REL and mx <= GATE_ABS, (what, rel, mx)


def _rel_residual(f, x):
    """rel of the reference's broyden at x: |f(x) - x| / (|(f(x) - x) + x| + 1e-9)."""
    g = f(x) - x
    return float(torch.norm(g)) / (float(torch.norm(g + x)) + 1e-9)


def _ae(sd, which):
    return [sd[f"autoencoder.{which}.mlp.mlp.{i}.{p}"] for i, p in ((0, "weight"), (0, "bias"), (2, "weight"), (2, "bias"))]


class Problem:
    """One mesh with one state dict: the float64 oracle side (CPU) and the device handles, both made once."""

    def __init__(self, mesh, sd, dev, tile_target=0, h0=None):
        eng = self.eng = pkg("engine")
        self.mesh, self.sd, self.dev = mesh, sd, dev
        self.s64, self.m64 = _to64(sd, mesh)
        with float64_default(), torch.no_grad():
            self.h0 = orc.encoder(self.s64, self.m64.x) if h0 is None else h0
        self.md = mesh.to(dev)
        self.plan = eng.MeshPlan(self.md, tile_target=tile_target)
        self.w = eng.PackedWeights64(sd, dev)
        self.fmap = eng.FixedPointMap64(self.plan, self.w, self.h0.to(dev), self.md.prb_data, self.md.edge_attr,
                                        getattr(self.md, "unit_normal_vector", None))
        self._solvers = {}

    def f_cpu(self, H):
        with float64_default(), torch.no_grad():
            return orc.function_forward(self.s64, H.clone(), self.h0, self.m64)

    def solver(self, threshold):
        if threshold not in self._solvers:
            self._solvers[threshold] = self.eng.DeviceBroyden64(self.fmap, threshold)
        return self._solvers[threshold]

    def broyden_cpu(self, x0, threshold, eps):
        with float64_default(), torch.no_grad():
            return orc.broyden(lambda H: orc.function_forward(self.s64, H, self.h0, self.m64), x0.clone(), threshold=threshold, eps=eps)


_cache = {}


def fixture_problem(name, dev):
    if name not in _cache:
        g, mesh = load_case(name)
        p = Problem(mesh, load_weights(CASES[name]), dev)
        p.golden = g
        _cache[name] = p
    return _cache[name]


def converged(name, dev):
    """The device solve every fixture test shares: from h0, eps 1e-11, threshold 1000."""
    key = ("solve", name)
    if key not in _cache:
        p = fixture_problem(name, dev)
        _cache[key] = p.solver(1000).solve(p.h0.to(dev), 1e-11)
        o = _cache[key]
        print(f"F64 {name}: n_iter {o['n_iter']} nstep {o['nstep']} lowest {o['lowest']:.3e} stop {o['stop_reason']}")
    return _cache[key]


# ----------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("name", FIXTURES)
def test_single_f_and_mlp(name, dev):
    p = fixture_problem(name, dev)
    enc = p.eng.mlp2_64(p.md.x, *_ae(p.sd, "encoder"))
    assert enc.dtype == torch.float64
    _close(enc, p.h0, f"{name} encoder")
    got = p.fmap(p.h0.to(dev))
    assert got.dtype == torch.float64 and got.shape == p.h0.shape
    _close(got, torch.from_numpy(p.golden["fp64_f1"]), f"{name} f(h0) vs stored fp64_f1")
    assert torch.equal(got, p.fmap(p.h0.to(dev)))   # fixed summation order: the same call gives the same bits


# ----------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("case", ["slots255_split", "ragged65", "slots256"])
def test_structure_limits(case, mixed, dev):
    c = lg.build(case, mixed)
    N = c.mesh.num_nodes
    gen = torch.Generator().manual_seed(21)
    H = 0.3 * torch.randn(N, 10, generator=gen, dtype=torch.float64)
    H0 = 0.3 * torch.randn(N, 10, generator=gen, dtype=torch.float64)
    p = Problem(c.mesh, load_weights("mixed" if mixed else "dirichlet"), dev, tile_target=c.tile_target, h0=H0)
    assert p.plan.tiled == c.tiled, (case, p.plan.tiled)
    if case == "slots256":
        assert not p.plan.tiled
    _close(p.fmap(H.to(dev)), p.f_cpu(H), f"{case}-{'mixed' if mixed else 'dirichlet'} f")


# ----------------------------------------------------------------------------------------------------------------- 3
def _random_two_layer_mixed(seed=5):
    """``_random_two_layer`` for the mixed family."""
    torch.manual_seed(seed)
    net = pkg("mixed").ModelPSIGNN(dict(latent_dim=10, n_layers=2))
    for q in net.parameters():
        if q.dim() == 1:
            torch.nn.init.normal_(q, std=0.1)
    return {k: v.detach().clone() for k, v in net.state_dict().items()}


@pytest.mark.parametrize("mixed", [False, True])
def test_two_layer_block(mixed, dev):
    """n_layers = 2: the dirichlet chain (no LayerNorm on the first layer, Dirichlet rows reset after each) and the mixed family's
    loop that never reassigns h."""
    _, mesh = load_case("hex13_mixed_s1" if mixed else "hex13_dirichlet_s0")
    sd = _random_two_layer_mixed() if mixed else _random_two_layer()
    gen = torch.Generator().manual_seed(22)
    H = 0.3 * torch.randn(mesh.num_nodes, 10, generator=gen, dtype=torch.float64)
    H0 = 0.3 * torch.randn(mesh.num_nodes, 10, generator=gen, dtype=torch.float64)
    p = Problem(mesh, sd, dev, h0=H0)
    assert p.w.n_layers == 2 and p.w.mixed == mixed
    _close(p.fmap(H.to(dev)), p.f_cpu(H), f"two layers {'mixed' if mixed else 'dirichlet'} f")


# ----------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("name", FIXTURES)
def test_first_iterations(name, dev):
    p = fixture_problem(name, dev)
    got = converged(name, dev)
    want = p.broyden_cpu(p.h0, 10, 1e-11)
    assert got["n_iter"] >= 10
    for tr in ("rel_trace", "abs_trace"):
        a, b = np.array(got[tr][:10]), np.array(want[tr][:10])
        print(f"F64 {name} {tr}[:10] max rel diff {float(np.max(np.abs(a - b) / b)):.2e}")
        np.testing.assert_allclose(a, b, rtol=1e-9, atol=0)


# ----------------------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("name", FIXTURES + ["hex26_dirichlet_s0"])
def test_converged_against_stored_truth(name, dev):
    p = fixture_problem(name, dev)
    out = converged(name, dev)
    dist = rel_l2(out["result"], p.golden["fp64_result"])
    print(f"F64 {name}: lowest {out['lowest']:.3e}, distance to the stored fp64_result {dist:.2e}")
    assert out["lowest"] < 1e-11
    assert dist <= 5e-9
    assert out["result"].dtype == torch.float64 and not out["prot_break"]
    u = p.eng.mlp2_64(out["result"], *_ae(p.sd, "decoder"))
    with float64_default(), torch.no_grad():
        want_u = orc.decoder(p.s64, out["result"].cpu())
    d = rel_l2(u, want_u)
    print(f"F64 {name}: decoder rel L2 {d:.2e}")
    assert d <= 1e-13


# ----------------------------------------------------------------------------------------------------------------- 6
@pytest.mark.parametrize("name", ["hex13_dirichlet_s0", "hex13_mixed_s1"])
def test_tight(name, dev):
    p = fixture_problem(name, dev)
    x0 = torch.from_numpy(p.golden["fp64_result"])
    out = p.solver(200).solve(x0.to(dev), 1e-13)
    want = p.broyden_cpu(x0, 200, 1e-13)
    res = _rel_residual(p.f_cpu, out["result"].cpu())
    dist = rel_l2(out["result"], want["result"])
    print(f"F64 tight {name}: device lowest {out['lowest']:.3e} after {out['n_iter']} steps (oracle {want['lowest']:.3e}, "
          f"nstep {want['nstep']}); oracle's residual of the device result {res:.3e}; distance {dist:.3e}")
    assert out["lowest"] <= 1e-13
    assert res <= 2e-13
    assert dist <= 50 * (out["lowest"] + want["lowest"])


# ----------------------------------------------------------------------------------------------------------------- 7
def test_same_bits(dev):
    name = "hex13_dirichlet_s0"
    p = fixture_problem(name, dev)
    first = converged(name, dev)
    sv, x0 = p.solver(1000), p.h0.to(dev)
    runs = {"second solve, same handle": sv.solve(x0, 1e-11), "poll_every 1": sv.solve(x0, 1e-11, poll_every=1),
            "poll_every 64": sv.solve(x0, 1e-11, poll_every=64)}
    for what, o in runs.items():
        assert torch.equal(o["result"], first["result"]), what
        assert (o["nstep"], o["n_iter"]) == (first["nstep"], first["n_iter"]), what
        assert o["rel_trace"] == first["rel_trace"] and o["abs_trace"] == first["abs_trace"], what


# ----------------------------------------------------------------------------------------------------------------- 8
@pytest.mark.parametrize("mixed", [False, True])
def test_many_blocks_ragged_tail(mixed, dev):
    """10 981 nodes: 109 810 elements are 215 blocks of 512 and 108 chunks of 1 024, both with a ragged tail.  No claim about
    convergence; what the solver reports must be what its result has."""
    mesh = pkg("data").make_hex_problem(60, seed=3, mixed=mixed, compute_sol=False)
    assert mesh.num_nodes == 10981
    p = Problem(mesh, load_weights("mixed" if mixed else "dirichlet"), dev)
    _close(p.fmap(p.h0.to(dev)), p.f_cpu(p.h0), f"hex60 {'mixed' if mixed else 'dirichlet'} f(h0)")
    out = p.solver(300).solve(p.h0.to(dev), 1e-9)
    res = _rel_residual(p.f_cpu, out["result"].cpu())
    print(f"F64 hex60 {'mixed' if mixed else 'dirichlet'}: n_iter {out['n_iter']} nstep {out['nstep']} lowest {out['lowest']:.3e} "
          f"oracle's residual of the result {res:.3e} stop {out['stop_reason']}")
    np.testing.assert_allclose(out["lowest"], res, rtol=1e-6)
    # nstep is the reference's 1-based step of the lowest iterate; entry i of the trace is the residual after step i + 1
    trace = out["rel_trace"]
    assert 1 <= out["nstep"] <= out["n_iter"] <= 300 and len(trace) == 301
    assert trace[out["nstep"] - 1] == out["lowest"] == min(trace)
