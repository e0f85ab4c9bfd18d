"""GPU: the float64 Newton-Krylov solver on the device (``psignn_gmres64_solve_shifted``, ``psignn_newton64_*``;
``engine.DeviceGmres64.solve_shifted``, ``DeviceNewton64``, ``fixed_point64(solver="newton")``).

The linear solve is compared with its torch restatement ``newton64_ref.gmres_shifted`` driven by the float64 CPU oracle's autograd
products (``newton64_ref.LinearProblem``: the state is the fixture's stored ``fp64_result``, ``b = randn`` seed 0).  Where the gates
come from (the rule of tests/test_gpu_f64.py): scripts/calib_f64_newton.py runs the restatement again with the oracle's edge list
permuted, three seeds -- the summation order is the only freedom a correct float64 statement has.  eta 1e-2, m 50, budget 200:

======================  =====  ================================  ================================  ==============================
case                    shift  J: products/cycles/stop/n_reorth  J^T                               result moved (J; J^T)
======================  =====  ================================  ================================  ==============================
hex13_dirichlet_s0      1.0    9 / 2 / tolerance / 7             9 / 2 / tolerance / 7             4.1e-16; 4.2e-16
hex13_dirichlet_s0      1.5    4 / 2 / tolerance / 2             4 / 2 / tolerance / 2             5.4e-17; 6.0e-17
hex13_mixed_s1          1.0    20 / 2 / tolerance / 17           14 / 2 / tolerance / 11           4.0e-15; 9.2e-16
hex13_mixed_s1          1.5    5 / 2 / tolerance / 2             5 / 2 / tolerance / 2             8.0e-17; 1.1e-16
two layers dirichlet    1.0    4 / 2 / tolerance / 1             4 / 2 / tolerance / 1             1.1e-16; 1.3e-16
two layers dirichlet    1.5    4 / 2 / tolerance / 1             4 / 2 / tolerance / 1             7.3e-17; 8.7e-17
two layers mixed        1.0    3 / 2 / tolerance / 1             3 / 2 / tolerance / 1             4.2e-17; 5.0e-17
two layers mixed        1.5    3 / 2 / tolerance / 1             3 / 2 / tolerance / 1             3.7e-17; 4.2e-17
======================  =====  ================================  ================================  ==============================

No count moved in any permuted run with seed 0 for ``b``, so that is the seed of every case.

* the result (test 1): relative L2 <= 9.9e-13 of the restatement's, 250 x the worst movement above (3.95e-15).
* the residual (tests 1, 3, 4): ``|shift d - A d - b| / |b|`` recomputed with ``FixedPointMap64.jvp`` / ``.vjp`` is <= eta when the
  stop reason is tolerance, and may exceed what the solve reports by rtol 1e-4, the margin tests/test_gpu_f64_adjoint.py gives the
  recomputed residual of a converged solve.
* duality (test 2): both orientations to eta 1e-12 at shift 1.5.  ``a = <w, d_forward(b)>`` and ``c = <d_transposed(w), b>`` differ
  by ``<r_t, d_f> - <d_t, r_f>``; the figure is ``|a - c| / (|w| |d_f| + |d_t| |b|)``.  The restatement's own figure is at most
  5.28e-15 (hex13_mixed_s1; 4.4e-15, 1.1e-15, 1.4e-16 on the others; the permuted runs move it in the third digit); the gate
  1.3e-12 is 250 x that.
* the outer loop (test 5): the gates this solver was specified with -- stop reason tolerance within 40 attempted steps at eps 1e-11,
  the result within 5e-9 relative L2 of the stored ``fp64_result`` (the gate, and its derivation, of test 5 of
  tests/test_gpu_f64.py), every accepted sigma = 0 step from 1e-10 <= rel < 1e-6 cutting ``|g|`` at least 10 x (a float64 CPU run
  with scipy's GMRES gave 110 - 153 x at eta 1e-2), ``rel`` recomputed from ``result`` equal to ``lowest`` at rtol 1e-6 (the same
  ``f`` kernel on the same state: only the order of the norm's sum differs).

The inner target of the linear solve is ``|g_{j+1}| <= eta |b|``, not the ``eps / 2`` of the adjoint solve.  The limits of test 5
come from a float64 CPU run of the outer loop around scipy's GMRES, which ends a cycle at ``eta |b|``; the CPU restatement of this
file with that target reproduces that run's steps and products on all seven runs (8 / 173, 23 / 347, 8 / 219, 13 / 270, 14 / 270,
17 / 250, 17 / 579).  With ``eta / 2`` hex26 needs 41 steps and 1 115 products (measured on the device and on the CPU, digit for
digit): oversolving steps 5 - 8 leads into 25 steps at sigma 0.01 - 0.04 that gain a few percent each.

On the MI355X, one run: every count of test 1 equal to the restatement's, results 1.0e-16 - 4.1e-15 from it (worst: hex13_mixed_s1,
shift 1, J); duality gaps 4.45e-15 / 5.28e-15 / 1.11e-15 / 1.45e-16, the restatement's own; the outer loop from h0 at eps 1e-11:

======================  ======  ===============  ========  =========  =========  ==============================
fixture                 sigma0  attempted steps  rejected  products   lowest     distance to stored fp64_result
======================  ======  ===============  ========  =========  =========  ==============================
hex13_dirichlet_s0      0       8                0         173        2.2e-13    9.4e-11
hex13_dirichlet_s0      1       23               1         347        3.8e-13    1.0e-10
hex13_mixed_s1          0       8                0         219        9.0e-13    1.5e-10
hex13_mixed_s1          1       13               0         270        7.9e-12    6.2e-10
original_dirichlet_s0   0       14               1         270        5.4e-13    1.2e-10
original_dirichlet_s0   1       17               0         250        6.9e-13    1.2e-10
hex26_dirichlet_s0      0       17               1         579        1.4e-12    5.0e-10
======================  ======  ===============  ========  =========  =========  ==============================

These are the steps, products, residuals and distances of the CPU run the limits were taken from, row for row.  ``|g|`` is cut
41 - 128 x on the sigma = 0 steps from 1e-10 <= rel < 1e-6.
"""
import math
import types

import numpy as np
import pytest
import torch

import handle_reuse as hr
import limit_graphs as lg
import newton64_ref as ref
import vjp_backward_cases as vb
from conftest import load_weights, pkg, rel_l2
from test_gpu_f64 import Problem, _ae, fixture_problem

pytestmark = pytest.mark.gpu

ETA = 1e-2
GATE_RESULT = 9.9e-13   # 250 x 3.95e-15
GATE_DUAL = 1.3e-12     # 250 x 5.28e-15
RES_MARGIN = 1e-4
_cache = {}


class Lin:
    """One linear problem on the CPU oracle and the device map of the same mesh and weights."""

    def __init__(self, name, dev):
        self.lp = lp = ref.LinearProblem(name)
        self.dp = Problem(lp.mesh, lp.sd, dev, h0=lp.h0)
        self.H, self.b, self.w = lp.H.to(dev), lp.b.to(dev), lp.w.to(dev)
        self.gm = self.dp.eng.DeviceGmres64(self.dp.fmap, 50)


def lin(name, dev):
    if name not in _cache:
        _cache[name] = Lin(name, dev)
    return _cache[name]


def true_rel(fmap, H, b, d, shift, transposed):
    """|shift d - A d - b| / |b| with the map's own products."""
    Ad = fmap.vjp(H, d) if transposed else fmap.jvp(H, d)
    return float((shift * d - Ad - b).norm()) / float(b.norm())


def check_residual(what, fmap, H, b, out, shift, transposed, eta):
    res = true_rel(fmap, H, b, out["result"], shift, transposed)
    print(f"F64N {what}: products {out['nstep']} cycles {out['n_cycles']} stop {out['stop']} n_reorth {out['n_reorth']} "
          f"lowest {out['lowest']:.6e} recomputed {res:.6e}")
    assert bool(torch.isfinite(out["result"]).all()) and math.isfinite(out["lowest"])
    assert out["lowest"] == min(out["rel_trace"]) and len(out["rel_trace"]) == out["n_cycles"]
    assert res <= out["lowest"] * (1 + RES_MARGIN) + 1e-300
    if out["stop"] == "tolerance":
        assert out["lowest"] <= eta and res <= eta * (1 + RES_MARGIN)
    return res


def rel_of(fmap, x):
    f = fmap(x)
    return float((f - x).norm()) / (float(f.norm()) + 1e-9)


def check_newton_traces(eng, out, kw=None):
    """The traces of one solve are self-consistent and obey ``psignn_newton64_policy`` replayed on them."""
    kw = kw or {}
    n = out["n_iter"]
    assert len(out["accepted"]) == len(out["krylov"]) == len(out["lin_stop"]) == len(out["trial_abs"]) == n
    assert len(out["sigma_trace"]) == n + 1
    assert len(out["rel_trace"]) == len(out["abs_trace"]) == 1 + sum(out["accepted"])
    assert out["n_products"] == sum(out["krylov"]) and out["n_feval"] == 1 + n
    assert out["lowest"] == min(out["rel_trace"]) and out["rel_trace"][out["nstep"]] == out["lowest"]
    sigma, g, k = out["sigma_trace"][0], out["abs_trace"][0], 0
    for i in range(n):
        acc, nxt = eng.newton64_policy(sigma, g, out["trial_abs"][i], kw.get("growth", 2.0), kw.get("reject_floor", 0.0625),
                                       kw.get("sigma_off", 1e-8))
        assert acc == out["accepted"][i] and nxt == out["sigma_trace"][i + 1], (i, acc, nxt, out["sigma_trace"][i + 1])
        if acc:
            k += 1
            assert out["abs_trace"][k] == out["trial_abs"][i]
            g = out["trial_abs"][i]
        sigma = nxt
    assert all(s in eng.GMRES_STOPS for s in out["lin_stop"]) and out["stop_reason"] in eng.NEWTON_STOPS


# ----------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("shift", ref.SHIFTS)
@pytest.mark.parametrize("name", ref.CASE_NAMES)
def test_shifted_solve_against_the_restatement(name, shift, transposed, dev):
    p = lin(name, dev)
    want = p.lp.solve(shift, transposed, eta=ETA, max_products=200, m=50)
    got = p.gm.solve_shifted(p.H, p.b, shift=shift, transposed=transposed, eta=ETA, max_products=200)
    dist = rel_l2(got["result"], want["result"])
    what = f"{name} shift {shift} {'J^T' if transposed else 'J'}"
    print(f"F64N {what}: restatement {want['nstep']} / {want['n_cycles']} / {want['stop']} / {want['n_reorth']} lowest "
          f"{want['lowest']:.6e}; distance {dist:.2e}")
    check_residual(what, p.dp.fmap, p.H, p.b, got, shift, transposed, ETA)
    assert got["result"].dtype == torch.float64 and got["result"].shape == p.lp.b.shape
    assert (got["nstep"], got["n_cycles"], got["stop"], got["n_reorth"]) == \
        (want["nstep"], want["n_cycles"], want["stop"], want["n_reorth"])
    assert dist <= GATE_RESULT


# ----------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("name", ref.CASE_NAMES)
def test_duality(name, dev):
    p = lin(name, dev)
    f = p.gm.solve_shifted(p.H, p.b, shift=1.5, transposed=False, eta=1e-12, max_products=2000)
    t = p.gm.solve_shifted(p.H, p.w, shift=1.5, transposed=True, eta=1e-12, max_products=2000)
    a, c = float((p.w * f["result"]).sum()), float((t["result"] * p.b).sum())
    scale = float(p.w.norm() * f["result"].norm() + t["result"].norm() * p.b.norm())
    gap = abs(a - c) / scale
    print(f"F64N {name} duality: <w, d_f> {a:.15e} <d_t, b> {c:.15e} normalised gap {gap:.2e}; products {f['nstep']} / {t['nstep']} "
          f"stops {f['stop']} / {t['stop']} lowest {f['lowest']:.2e} / {t['lowest']:.2e}")
    assert f["stop"] == t["stop"] == "tolerance"
    assert gap <= GATE_DUAL


# ----------------------------------------------------------------------------------------------------------------- 3
def _shapes_run(what, p, H, dev, seed=0, newton_kw=None):
    """Both orientations of the shifted solve with the residual check, b = 0, and one Newton solve from H."""
    eng = p.eng
    b = torch.randn(H.shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64).to(dev)
    gm = eng.DeviceGmres64(p.fmap, 20)
    try:
        for transposed in (False, True):
            for shift in (1.0, 1.5):
                out = gm.solve_shifted(H, b, shift=shift, transposed=transposed, eta=ETA, max_products=60)
                check_residual(f"{what} shift {shift} {'J^T' if transposed else 'J'}", p.fmap, H, b, out, shift, transposed, ETA)
                assert out["nstep"] <= 60
            z = gm.solve_shifted(H, torch.zeros_like(b), shift=1.5, transposed=transposed)
            assert z["nstep"] == 0 and z["n_cycles"] == 1 and z["stop"] == "tolerance" and z["lowest"] == 0.0
            assert not bool(z["result"].any())
    finally:
        gm.close()
    nt = eng.DeviceNewton64(p.fmap, 20)
    try:
        kw = dict(eps=1e-11, threshold=25, max_products=80)
        kw.update(newton_kw or {})
        out = nt.solve(H, **kw)
    finally:
        nt.close()
    rel = rel_of(p.fmap, out["result"])
    print(f"F64N {what} Newton: stop {out['stop_reason']} n_iter {out['n_iter']} accepted {sum(out['accepted'])} products "
          f"{out['n_products']} lowest {out['lowest']:.3e} recomputed {rel:.3e} sigma {out['sigma_trace']} lin {out['lin_stop']}")
    check_newton_traces(eng, out)
    assert bool(torch.isfinite(out["result"]).all()) and math.isfinite(rel)
    np.testing.assert_allclose(rel, out["lowest"], rtol=1e-6)
    assert (out["stop_reason"] == "tolerance") == (out["lowest"] < 1e-11)
    if out["stop_reason"] == "threshold":
        assert out["n_iter"] == kw["threshold"]
    if out["stop_reason"] == "rejects":
        assert out["accepted"][-8:] == [False] * 8
    return out


@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 128, 129])
def test_line_graphs(N, mixed, dev):
    """Lengths around the 64-lane wave and the 128-element half block; at N = 1 the map's ten elements are one short block and the
    Arnoldi process breaks down (|w| = 0) once the Krylov space is the whole space."""
    fam = "mixed" if mixed else "dirichlet"
    mesh = vb.line_graph(N, mixed)
    p = Problem(mesh, load_weights(fam), dev)
    _shapes_run(f"line{N} {fam}", p, p.h0.to(dev), dev, seed=N)


@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("case", ["slots255_split", "ragged65", "slots256"])
def test_structure_limits(case, mixed, dev):
    c = lg.build(case, mixed)
    fam = "mixed" if mixed else "dirichlet"
    gen = torch.Generator().manual_seed(21)
    H = 0.3 * torch.randn(c.mesh.num_nodes, 10, generator=gen, dtype=torch.float64)
    H0 = 0.3 * torch.randn(c.mesh.num_nodes, 10, generator=gen, dtype=torch.float64)
    p = Problem(c.mesh, load_weights(fam), dev, tile_target=c.tile_target, h0=H0)
    assert p.plan.tiled == c.tiled
    _shapes_run(f"{case} {fam}", p, H.to(dev), dev)


# ----------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("mixed", [False, True])
def test_many_blocks_ragged_tail(mixed, dev):
    """10 981 nodes at the encoder state: 109 810 elements are 215 blocks of 512 and 108 chunks of 1 024, both with a ragged tail.
    No claim about convergence of the Newton solve; what the solvers report must be what their results have."""
    sd, mesh, h0 = vb.hex60(mixed)
    p = Problem(mesh, sd, dev, h0=h0)
    out = _shapes_run(f"hex60 {'mixed' if mixed else 'dirichlet'}", p, h0.to(dev), dev, newton_kw=dict(threshold=6, max_products=60))
    assert out["n_iter"] >= 1


# ----------------------------------------------------------------------------------------------------------------- 5
OUTER = [(n, s) for n in ("hex13_dirichlet_s0", "hex13_mixed_s1", "original_dirichlet_s0") for s in (0.0, 1.0)] + \
    [("hex26_dirichlet_s0", 0.0)]


def newton(name, dev, m=50):
    key = ("newton", name, m)
    if key not in _cache:
        p = fixture_problem(name, dev)
        _cache[key] = p.eng.DeviceNewton64(p.fmap, m)
    return _cache[key]


@pytest.mark.parametrize("name,sigma0", OUTER)
def test_outer_loop_converges(name, sigma0, dev):
    p = fixture_problem(name, dev)
    out = newton(name, dev).solve(p.h0.to(dev), eps=1e-11, threshold=40, sigma0=sigma0)
    dist = rel_l2(out["result"], p.golden["fp64_result"])
    rel = rel_of(p.fmap, out["result"])
    print(f"F64N {name} sigma0 {sigma0}: stop {out['stop_reason']} n_iter {out['n_iter']} accepted {sum(out['accepted'])} products "
          f"{out['n_products']} lowest {out['lowest']:.3e} recomputed {rel:.3e} distance to the stored fp64_result {dist:.2e}")
    print(f"F64N {name} sigma0 {sigma0}: sigma {['%.3g' % s for s in out['sigma_trace']]} rel {['%.2e' % r for r in out['rel_trace']]} "
          f"krylov {out['krylov']} lin {sorted(set(out['lin_stop']))}")
    check_newton_traces(p.eng, out)
    assert out["stop_reason"] == "tolerance" and out["lowest"] < 1e-11 and out["n_iter"] <= 40
    assert out["result"].dtype == torch.float64 and out["result"].shape == p.h0.shape
    assert dist <= 5e-9
    np.testing.assert_allclose(rel, out["lowest"], rtol=1e-6)
    # plain inexact Newton near the solution: an accepted sigma = 0 step from 1e-10 <= rel < 1e-6 cuts |g| at least 10 x
    k, cuts = 0, []
    for i, acc in enumerate(out["accepted"]):
        if not acc:
            continue
        if out["sigma_trace"][i] == 0.0 and 1e-10 <= out["rel_trace"][k] < 1e-6:
            cuts.append(out["abs_trace"][k] / out["abs_trace"][k + 1])
        k += 1
    print(f"F64N {name} sigma0 {sigma0}: |g| cut by {['%.1f' % c for c in cuts]} on the sigma = 0 steps from 1e-10 <= rel < 1e-6")
    assert all(c >= 10.0 for c in cuts), cuts


# ----------------------------------------------------------------------------------------------------------------- 6
def test_reject_path(dev):
    """growth 1e-3 rejects every step that does not cut |g| a thousandfold: three rejections in a row end the solve, sigma goes
    0 -> 1/16 -> 1/4 -> 1, and the state is untouched bit for bit."""
    name = "hex13_dirichlet_s0"
    p = fixture_problem(name, dev)
    x0 = p.h0.to(dev)
    kw = dict(growth=1e-3, sigma0=0.0, max_rejects=3)
    out = newton(name, dev).solve(x0, eps=1e-11, threshold=40, **kw)
    print(f"F64N reject path: stop {out['stop_reason']} sigma {out['sigma_trace']} trial |g| {out['trial_abs']} |g0| {out['abs_trace']}")
    check_newton_traces(p.eng, out, kw)
    assert out["stop_reason"] == "rejects" and out["accepted"] == [False] * 3 and out["n_iter"] == 3
    assert out["sigma_trace"] == [0.0, 0.0625, 0.25, 1.0]
    assert hr.same_tensor(out["result"], x0) and out["nstep"] == 0 and len(out["rel_trace"]) == 1
    assert out["lowest"] == out["rel_trace"][0]
    np.testing.assert_allclose(out["lowest"], rel_of(p.fmap, x0), rtol=1e-6)


# ----------------------------------------------------------------------------------------------------------------- 7
def test_same_bits(dev):
    name = "hex13_dirichlet_s0"
    p = fixture_problem(name, dev)
    x0 = p.h0.to(dev)
    other = 0.5 * x0 + 0.5 * torch.from_numpy(p.golden["fp64_result"]).to(dev)
    run_b = lambda h: h.solve(x0, eps=1e-11, threshold=40)
    run_a = lambda h: h.solve(other, eps=1e-9, threshold=40, sigma0=0.0)
    chain = hr.Reused("newton64", lambda: p.eng.DeviceNewton64(p.fmap, 50))
    try:
        first = chain.link("from h0", run_b)
        hr.same_out(run_b(chain.h), first, "twice on one handle")
        chain.link("from a midpoint, sigma0 0", run_a)            # A, different from B
        hr.same_out(chain.link("from h0 after A", run_b), first, "B after A against the first B")
        for pe in (1, 8, 1000):
            hr.same_out(chain.h.solve(x0, eps=1e-11, threshold=40, poll_every=pe), first, f"poll_every {pe}")
        assert chain.pairs >= 2
    finally:
        chain.close()
    # float64 inputs are the float32 ones widened; the linear solve keeps its bits on a reused handle too
    q = lin(name, dev)
    a = q.gm.solve_shifted(q.H, q.b, shift=1.5)
    q.gm.solve_shifted(q.H, q.w, shift=1.0, transposed=True)
    q.gm.solve_adjoint(q.H, q.b, 1e-11, 200)
    for pe in (1, 8, 1000):
        hr.same_out(q.gm.solve_shifted(q.H, q.b, shift=1.5, poll_every=pe), a, f"solve_shifted poll_every {pe}")
    fresh = q.dp.eng.DeviceGmres64(q.dp.fmap, 50)
    try:
        hr.same_out(fresh.solve_shifted(q.H, q.b, shift=1.5), a, "solve_shifted on a fresh handle")
    finally:
        fresh.close()
    b32 = q.b.float()
    hr.same_out(q.gm.solve_shifted(q.H, b32, shift=1.5), q.gm.solve_shifted(q.H, b32.double(), shift=1.5), "float32 b widened")


# ----------------------------------------------------------------------------------------------------------------- 8
def test_fixed_point64_routes(dev):
    name = "hex13_dirichlet_s0"
    p = fixture_problem(name, dev)
    eng = p.eng
    md = p.mesh.to(dev)
    got = eng.fixed_point64(md, p.sd, solver="newton", threshold=40)
    # the convenience encodes h0 on the device; the stored problem's h0 is the oracle's: both are float64 statements of the encoder
    fm = eng.FixedPointMap64(p.plan, p.w, got["h0"], md.prb_data, md.edge_attr)
    nt = eng.DeviceNewton64(fm, 50)
    want = nt.solve(got["h0"], eps=1e-11, threshold=40, poll_every=16)
    nt.close()
    fm.close()
    for k in want:
        if k != "result":
            assert got[k] == want[k], k
    assert hr.same_tensor(got["result"], want["result"]) and got["stop_reason"] == "tolerance"
    assert hr.same_tensor(got["u"], eng.mlp2_64(got["result"], *_ae(p.sd, "decoder")))
    assert rel_l2(got["result"], p.golden["fp64_result"]) <= 5e-9
    # the default route is the Broyden solve it has always been
    base = eng.fixed_point64(md, p.sd)
    fm = eng.FixedPointMap64(p.plan, p.w, base["h0"], md.prb_data, md.edge_attr)
    by = eng.DeviceBroyden64(fm, 1000)
    direct = by.solve(base["h0"], 1e-11, 16)
    by.close()
    fm.close()
    assert hr.same_tensor(base["result"], direct["result"])
    for k in direct:
        if k != "result":
            assert base[k] == direct[k], k
    assert hr.same_tensor(base["h0"], got["h0"])
    with pytest.raises(pkg("_native").NativeError, match="solver must be"):
        eng.fixed_point64(md, p.sd, solver="anderson")


# ----------------------------------------------------------------------------------------------------------------- 9
def test_refusals_on_open_handles(dev):
    nat = pkg("_native")
    name = "hex13_dirichlet_s0"
    q = lin(name, dev)
    eng, fm, gm = q.dp.eng, q.dp.fmap, q.gm
    nt = eng.DeviceNewton64(fm, 10)
    N = q.H.shape[0]
    before_l = gm.solve_shifted(q.H, q.b, shift=1.5)
    before_n = nt.solve(q.H, eps=1e-9, threshold=5)
    bad_shapes = [torch.zeros(N, 8, device=dev), torch.zeros(N - 1, 10, device=dev), torch.zeros(N * 10, device=dev)]
    for bad in bad_shapes:
        with pytest.raises(nat.NativeError, match="h has shape"):
            gm.solve_shifted(bad, q.b)
        with pytest.raises(nat.NativeError, match="b has shape"):
            gm.solve_shifted(q.H, bad)
        with pytest.raises(nat.NativeError, match="x0 has shape"):
            nt.solve(bad)
    with pytest.raises(nat.NativeError, match="device tensors"):
        gm.solve_shifted(q.H.cpu(), q.b)
    with pytest.raises(nat.NativeError, match="device tensors"):
        nt.solve(q.H.cpu())
    for s in (0.999, 0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(nat.NativeError, match="shift must be"):
            gm.solve_shifted(q.H, q.b, shift=s)
    for v in (float("nan"), float("inf"), -1e-3):
        with pytest.raises(nat.NativeError, match="eta must be"):
            gm.solve_shifted(q.H, q.b, eta=v)
        with pytest.raises(nat.NativeError, match="eta must be"):
            nt.solve(q.H, eta=v)
        with pytest.raises(nat.NativeError, match="eps must be"):
            nt.solve(q.H, eps=v)
    with pytest.raises(nat.NativeError, match="max_products"):
        gm.solve_shifted(q.H, q.b, max_products=0)
    for w in (8, 16):   # a map of another width: refused by the Python layer before any native call
        other = types.SimpleNamespace(handle=fm.handle, device=fm.device, weights=types.SimpleNamespace(width=w, n_layers=1))
        with pytest.raises(nat.NativeError, match="forward inference only"):
            eng.DeviceNewton64(other, 10)
        g2 = eng.DeviceGmres64.__new__(eng.DeviceGmres64)
        g2.fmap, g2.m, g2.device, g2.handle = other, 10, fm.device, gm.handle
        with pytest.raises(nat.NativeError, match="forward inference only"):
            g2.solve_shifted(q.H, q.b)
    # the C entry points say no with a code and a message: a workspace that is too small names its bytes, a shift below 1
    lib = nat.lib()
    need = max(lib.psignn_f64_deriv_workspace_doubles(fm.handle, 1, 0), lib.psignn_f64_deriv_workspace_doubles(fm.handle, 1, 1))
    work = torch.zeros(need, dtype=torch.float64, device=dev)
    out, info = torch.zeros_like(q.b), nat.GmresAdjointInfo()
    args = lambda n, shift=1.5: (gm.handle, nat.ptr(fm.wflat), 1, nat.ptr(q.H), nat.ptr(fm.h0), nat.ptr(fm.prb), None, nat.ptr(q.b),
                                 shift, 0, ETA, 20, 8, nat.ptr(work), n, nat.ptr(out), info, None, None, None)
    assert lib.psignn_gmres64_solve_shifted(*args(need - 1)) < 0
    assert f"{need * 8} bytes" in lib.psignn_last_error().decode()
    assert lib.psignn_gmres64_solve_shifted(*args(need, 0.5)) < 0 and "shift" in lib.psignn_last_error().decode()
    assert lib.psignn_gmres64_solve_shifted(*args(need)) == 0 and info.products <= 20
    with pytest.raises(nat.NativeError, match="restart length out of range"):
        eng.DeviceNewton64(fm, 4097)
    # every handle still works, and gives the bits it gave before
    hr.same_out(gm.solve_shifted(q.H, q.b, shift=1.5), before_l, "the linear solve after the refusals")
    hr.same_out(nt.solve(q.H, eps=1e-9, threshold=5), before_n, "the Newton solve after the refusals")
    assert nt.nbytes >= (11 + 6) * q.H.numel() * 8
    nt.close()
    with pytest.raises(nat.NativeError, match="closed"):
        nt.solve(q.H)
    closed = eng.DeviceGmres64(fm, 5)
    closed.close()
    with pytest.raises(nat.NativeError, match="closed"):
        closed.solve_shifted(q.H, q.b)
