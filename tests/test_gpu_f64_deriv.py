"""GPU: the float64 derivative products on the device (``psignn_f64_jvp``, ``psignn_f64_vjp``; ``engine.FixedPointMap64.jvp`` /
``.vjp``) against autograd on the CPU oracle in float64 (``orc.function_jvp`` / ``function_vjp``).

Where the gates come from.  The rule is that of tests/test_gpu_f64.py: about 250 x the float64 oracle's own spread when its edges are
permuted (the summation order is the only freedom a correct float64 statement has), which leaves room for the device's exp / sqrt
differing by a few ulp.  Measured on the CPU, v, w = randn, outputs O(1) - O(10):

=========================  ====================  ====================  ===================
graph                      J v   rel L2 / max    J^T w rel L2 / max    oracle duality gap
=========================  ====================  ====================  ===================
the three fixtures         <= 3.5e-16 / 8.9e-16  <= 4.1e-16 / 4.7e-16  0 - 6.4e-16
two layers, both families  <= 5.8e-16 / 1.7e-15  <= 5.8e-16 / 1.3e-15  5.0e-16 - 2.6e-14
slots255_split dirichlet   7.1e-17 / 2.2e-16     1.1e-16 / 5.6e-16     7.0e-16
slots255_split mixed       1.7e-16 / 1.4e-15     2.2e-16 / 1.2e-15     2.2e-15
ragged65 dirichlet         2.9e-16 / 3.3e-16     3.1e-16 / 5.2e-16     7.5e-16
ragged65 mixed             6.4e-16 / 4.9e-15     1.1e-15 / 5.3e-15     1.4e-16
slots256 dirichlet         9.3e-17 / 2.8e-16     2.6e-16 / 2.7e-15     5.9e-16
slots256 mixed             1.8e-16 / 1.8e-15     2.1e-16 / 1.0e-15     1.0e-15
hex60 (10 981) dirichlet   2.2e-16 / 6.7e-16     2.2e-16 / 4.4e-16     7.5e-16
hex60 (10 981) mixed       2.9e-16 / 8.9e-16     3.1e-16 / 4.4e-16     1.3e-15
=========================  ====================  ====================  ===================

* fixtures and two-layer blocks (tests 1, 3): relative L2 <= 1e-13, max-abs <= 1e-12, the gates of test_gpu_f64.py.  250 x the
  spread is 1.0e-13 / 2.2e-13 on the fixtures (at h0 and at the stored fp64_result) and 1.5e-13 / 4.2e-13 on the two-layer blocks;
  the round gates are kept, the tighter choice where they differ.
* structure limits (test 2): 250 x the worst spread of the table exceeds both, so the gates are those products: 250 x 1.06e-15 =
  2.7e-13 and 250 x 5.33e-15 = 1.4e-12 (ragged65 mixed, J^T w), for all six cases.
* duality (test 4): |<w, J v> - <J^T w, v>| / |<w, J v>| from the device's outputs, at most 250 x the oracle's own gap on the same
  mesh, state and vectors: 1.9e-13 (dirichlet), 3.2e-13 (mixed).
A ReLU mask differing between device and oracle would need a float64 pre-activation within ~1e-15 of zero; with ~1e6 of them that
has probability ~1e-8, so no case is left out and no cap is used.
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

import adjoint_gmres_ref as ref
import limit_graphs as lg
from conftest import GOLDEN, ROOT, load_case, load_weights, pkg, rel_l2
from oracle import psignn_oracle as orc
from test_gpu_f64 import FIXTURES, Problem, _random_two_layer_mixed, fixture_problem, float64_default
from test_gpu_plan_limits import _random_two_layer

pytestmark = pytest.mark.gpu

GATE = (1e-13, 1e-12)
GATE_LIMITS = (2.7e-13, 1.4e-12)
GATE_DUALITY = {False: 250 * 7.54e-16, True: 250 * 1.29e-15}


def _close(got, want, what, gate=GATE):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    rel, mx = rel_l2(got, want), float((got - want).abs().max())
    print(f"F64D {what}: rel L2 {rel:.2e} max-abs {mx:.2e}")
    assert rel <= gate[0] and mx <= gate[1], (what, rel, mx)


def _vw(shape, seed=31):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=gen, dtype=torch.float64), torch.randn(shape, generator=gen, dtype=torch.float64)


def _both_products(p, H, what, gate=GATE):
    """J v and J^T w of problem p at H against the oracle; returns the device's two outputs and the vectors."""
    v, w = _vw(H.shape)
    with float64_default():
        want_jv = orc.function_jvp(p.s64, H.clone(), p.h0, p.m64, v)
        want_jtw = orc.function_vjp(p.s64, H.clone(), p.h0, p.m64, w)
    Hd, vd, wd = H.to(p.dev), v.to(p.dev), w.to(p.dev)
    jv, jtw = p.fmap.jvp(Hd, vd), p.fmap.vjp(Hd, wd)
    assert jv.dtype == jtw.dtype == torch.float64 and jv.shape == jtw.shape == H.shape
    _close(jv, want_jv, f"{what} J v", gate)
    _close(jtw, want_jtw, f"{what} J^T w", gate)
    return jv, jtw, vd, wd


# ----------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("name", FIXTURES)
def test_products_on_the_fixtures(name, dev):
    p = fixture_problem(name, dev)
    for at, H in (("h0", p.h0), ("fp64_result", torch.from_numpy(p.golden["fp64_result"]))):
        jv, jtw, vd, wd = _both_products(p, H, f"{name} at {at}")
        Hd = H.to(dev)
        # fixed summation order: the same call gives the same bits; float32 inputs are widened exactly
        assert torch.equal(jv, p.fmap.jvp(Hd, vd)) and torch.equal(jtw, p.fmap.vjp(Hd, wd))
        assert torch.equal(p.fmap.jvp(Hd, vd.float()), p.fmap.jvp(Hd, vd.float().double()))
        # + add is the last operation of the row: the map of the adjoint system in one call
        assert torch.equal(p.fmap.vjp(Hd, wd, vd), jtw + vd)


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
    _both_products(p, H, f"{case}-{'mixed' if mixed else 'dirichlet'}", GATE_LIMITS)


# ----------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("mixed", [False, True])
def test_two_layer_block(mixed, dev):
    """n_layers = 2: the dirichlet chain (value and tangent through both layers; the stored state and the chain backwards; Dirichlet
    rows reset after each layer) and the mixed family's loop that never reassigns h."""
    _, mesh = load_case("hex13_mixed_s1" if mixed else "hex13_dirichlet_s0")
    sd = _random_two_layer_mixed() if mixed else _random_two_layer()
    gen = torch.Generator().manual_seed(22)
    H = 0.3 * torch.randn(mesh.num_nodes, 10, generator=gen, dtype=torch.float64)
    H0 = 0.3 * torch.randn(mesh.num_nodes, 10, generator=gen, dtype=torch.float64)
    p = Problem(mesh, sd, dev, h0=H0)
    assert p.w.n_layers == 2 and p.w.mixed == mixed
    jv, jtw, vd, wd = _both_products(p, H, f"two layers {'mixed' if mixed else 'dirichlet'}")
    assert torch.equal(jv, p.fmap.jvp(H.to(dev), vd)) and torch.equal(jtw, p.fmap.vjp(H.to(dev), wd))


# ----------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("mixed", [False, True])
def test_duality(mixed, dev):
    """10 981 nodes (43 blocks of 256 with a ragged tail), at the encoder state: <w, J v> and <J^T w, v> from the device's outputs."""
    mesh = pkg("data").make_hex_problem(60, seed=3, mixed=mixed, compute_sol=False)
    assert mesh.num_nodes == 10981
    p = Problem(mesh, load_weights("mixed" if mixed else "dirichlet"), dev)
    v, w = _vw(p.h0.shape)
    Hd, vd, wd = p.h0.to(dev), v.to(dev), w.to(dev)
    a, b = float((wd * p.fmap.jvp(Hd, vd)).sum()), float((p.fmap.vjp(Hd, wd) * vd).sum())
    gap = abs(a - b) / abs(a)
    print(f"F64D hex60 {'mixed' if mixed else 'dirichlet'}: <w, J v> {a:.15e} <J^T w, v> {b:.15e} gap {gap:.2e}")
    assert gap <= GATE_DUALITY[mixed]


# ----------------------------------------------------------------------------------------------------------------- 5
def test_refusals_on_an_open_handle(dev):
    """Aliasing, a layer count out of range and a workspace that is too small are error codes; the message names the bytes."""
    nat = pkg("_native")
    p = fixture_problem("hex13_dirichlet_s0", dev)
    fm, lib = p.fmap, nat.lib()
    N = p.plan.N
    need = lib.psignn_f64_deriv_workspace_doubles(fm.handle, 1, 1)
    assert need == 3 * N * 10 and lib.psignn_f64_deriv_workspace_doubles(fm.handle, 1, 0) == 0
    assert lib.psignn_f64_deriv_workspace_doubles(fm.handle, 3, 1) == (3 + 2 + 2) * N * 10
    assert lib.psignn_f64_deriv_workspace_doubles(fm.handle, 3, 0) == 4 * N * 10
    assert lib.psignn_f64_deriv_workspace_doubles(fm.handle, 0, 1) == -1
    H, x, out = (torch.zeros(N, 10, dtype=torch.float64, device=dev) for _ in range(3))
    work = torch.zeros(need, dtype=torch.float64, device=dev)
    ptr = nat.ptr
    jvp = lambda nl, h, v, o: lib.psignn_f64_jvp(fm.handle, ptr(fm.wflat), nl, ptr(h), ptr(fm.h0), ptr(fm.prb), None, ptr(v), ptr(o),
                                                 None, 0, None)
    vjp = lambda nl, h, w, a, o, n: lib.psignn_f64_vjp(fm.handle, ptr(fm.wflat), nl, ptr(h), ptr(fm.h0), ptr(fm.prb), None, ptr(w),
                                                       a, ptr(o), ptr(work), n, None)
    assert jvp(1, H, x, H) < 0 and "alias" in lib.psignn_last_error().decode()
    assert jvp(1, H, x, x) < 0 and jvp(0, H, x, out) < 0 and jvp(65, H, x, out) < 0
    assert vjp(1, H, x, None, H, need) < 0 and "alias" in lib.psignn_last_error().decode()
    assert vjp(1, H, x, None, x, need) < 0 and vjp(1, H, x, ptr(out), out, need) < 0 and vjp(0, H, x, None, out, need) < 0
    assert vjp(1, H, x, None, out, need - 1) < 0
    assert f"{need * 8} bytes" in lib.psignn_last_error().decode()
    assert vjp(1, H, x, None, out, need) == 0
    torch.cuda.synchronize(dev)


# ----------------------------------------------------------------------------------------------------------------- 6
def test_same_bits_as_the_recorded_build(dev):
    """tests/golden/f64_deriv_parent.npz (scripts/record_f64_deriv_golden.py, recorded on the commit before W64, the handle and the
    LayerNorm backward of csrc/fgnn_f64_deriv.hip were each stated once): J v, J^T w (with and without add), the J^T w of the
    parameter VJP and the whole flat parameter gradient, on the three adjoint fixtures and the two-layer chain, bit for bit."""
    spec = importlib.util.spec_from_file_location("record_f64_deriv_golden", os.path.join(ROOT, "scripts", "record_f64_deriv_golden.py"))
    rec = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rec)
    want = np.load(os.path.join(GOLDEN, "f64_deriv_parent.npz"))
    assert tuple(rec.CASES)[:3] == ref.FIXTURES
    seen = set()
    for name in rec.CASES:
        for key, got in rec.run_case(name, dev).items():
            assert np.array_equal(got, want[f"{name}.{key}"]), (name, key)
            seen.add(f"{name}.{key}")
    assert seen == set(want.files)
