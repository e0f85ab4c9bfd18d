"""GPU: augmented restarts (LGMRES) and the stall ratio of the float64 GMRES on the device (``psignn_gmres64_create_aug``,
``psignn_gmres64_solve_*_opts``, ``psignn_newton64_create_aug``, ``psignn_newton64_solve_opts``; ``engine.DeviceGmres64Aug``,
``DeviceNewton64Aug``, ``adjoint64_aug``) against the restatement ``lgmres_ref.lgmres_adjoint``.

The restatement runs in float64 on the device with the map's own ``FixedPointMap64.vjp`` / ``.jvp`` as its operator, so the products
have the device's bits and only the order of the sums of the dots, norms and combinations differs.  Where the gates come from (the
rule of tests/test_gpu_f64.py): scripts/calib_f64_lgmres.py runs the restatement on the float64 CPU oracle again with every product
multiplied element by element by 1 + s * 2^-52, s uniform in [-4, 4], three seeds -- the freedom a correct float64 statement with
another summation order has -- on the runs of tests 2, 4 and 5:

=====================================================  ==================  ==============  =========================
runs                                                   a count moved       result moved    trace entries moved (abs)
=====================================================  ==================  ==============  =========================
test 2: 3 fixtures, m 10, augment 1 / 2, budget 60     in 0 of 6 runs      <= 6.10e-15     <= 1.1e-14
test 4: shifted, m 8, augment 2, eta 1e-8, 4 runs      in 0 of 4 runs      <= 3.99e-15     <= 6.5e-15
test 5: lines of 1 .. 129 nodes, m 4, augment 3        in 0 of 30 runs     <= 8.05e-15     <= 7.1e-15
=====================================================  ==================  ==============  =========================

(test 2: 60 products / 7 cycles / n_aug 5 with augment 1, 9 with augment 2 / budget on every fixture: stored corrections 0, 1, 2, a
wrapping ring, and a last cycle of left = 4, so ka = 2, nk = 2.)  The gates are 250 x these: the result within 1.6e-12 / 1.0e-12 /
2.1e-12 relative L2 of the restatement's, every trace entry within 2.8e-12 / 1.7e-12 / 1.8e-12 absolute (the large entries, |grad| ~
1e2, move by 1e-14; the relative movement of the small ones, up to 5e-9 on an entry at 1e-8, is the same absolute movement).  Products,
cycles, ``n_aug``, the stop reason and ``n_reorth`` are equal.

* test 3: what tests/test_host_lgmres.py asks of the restatement on the CPU oracle, asked of the device.
* test 4, independently: ``|shift d - A d - b| / |b|`` recomputed with the map's own products equals the reported ``lowest`` to 1e-6
  relative and is <= eta.
* test 5: m = 4, augment = 3 -- from the fourth cycle on a cycle is one Krylov step and three augmentation steps.  Budgets 5 c + 2 and
  5 c + 3 give cycle c a ``left`` of 1 (ka = 0) and 2 (ka = 1) when the cycles before it were full; c = 1, 2, 3.  On 51 and 103 nodes
  a cycle raises ``rel`` and the solve ends on stagnation before cycle 3; the device must end as the restatement does.
* test 7: the gate of tests/test_gpu_f64_newton.py for the default solver: stop reason tolerance at eps 1e-11, the result within 5e-9
  relative L2 of the stored ``fp64_result``.

On the MI355X, one run: every count equal to the restatement's in all 40 runs of tests 2, 4 and 5; results 6.5e-16 - 4.9e-15 (test
2), 9.1e-17 - 1.6e-15 (test 4) and at most 4.7e-15 (test 5, 51 nodes) from the restatement's; trace entries within 1.4e-14 absolute
(test 2, on |grad| = 145), 3.4e-15 (test 4) and 7.1e-15 (test 5).  Test 3, m = 10, products with augment 0 / 1 / 2:
hex13_dirichlet_s0 207 / 121 / 132, hex26_dirichlet_s0 605 / 242 / 241, hex13_mixed_s1 341 / 176 / 208, errors to ``truth()``
3.7e-9 - 4.0e-8 plain and 1.7e-9 - 1.5e-8 augmented (the largest ratio 2.9, hex13_dirichlet_s0 with one kept correction); today's
rule stops hex26 after 55 products at 2.1e-4 and hex13_mixed_s1 after 44 at 6.8e-4.  Test 7: 22 / 14 attempted steps, 393 / 399
products, 1.0e-10 / 1.5e-10 from the stored ``fp64_result``."""
import ctypes
import math

import numpy as np
import pytest
import torch

import adjoint_gmres_ref as ref
import handle_reuse as hr
import lgmres_ref as lg
import vjp_backward_cases as vb
from conftest import load_weights, pkg, rel_l2
from test_gpu_f64 import Problem, fixture_problem
from test_gpu_f64_adjoint import pair
from test_gpu_f64_newton import lin, true_rel

pytestmark = pytest.mark.gpu

EPS = 1e-10
GATE = {2: (1.6e-12, 2.8e-12), 4: (1.0e-12, 1.7e-12), 5: (2.1e-12, 1.8e-12)}   # test: (result, rel L2; trace entries, absolute)
COUNTS = ("nstep", "n_cycles", "n_aug", "stop", "n_reorth")
_handles, _runs = {}, {}


def handle(p, m, augment):
    """The ``DeviceGmres64Aug`` of a ``Pair`` / ``Lin``, made once."""
    key = (id(p), m, augment)
    if key not in _handles:
        _handles[key] = p.dp.eng.DeviceGmres64Aug(p.dp.fmap, m, augment)
    return _handles[key]


def against_restatement(what, got, want, test):
    g_res, g_tr = GATE[test]
    dist = rel_l2(got["result"], want["result"]) if float(want["result"].norm()) else float(got["result"].norm())
    print(f"LGM {what}: device {' / '.join(str(got[k]) for k in COUNTS)} lowest {got['lowest']:.6e}; restatement "
          f"{' / '.join(str(want[k]) for k in COUNTS)} lowest {want['lowest']:.6e}; distance {dist:.2e}")
    for tr in ("rel_trace", "abs_trace"):
        a, b = np.array(got[tr]), np.array(want[tr])
        print(f"LGM {what} {tr}: max |a - b| {float(np.max(np.abs(a - b))) if a.shape == b.shape else float('nan'):.2e}")
    assert tuple(got[k] for k in COUNTS) == tuple(want[k] for k in COUNTS)
    assert got["result"].dtype == torch.float64 and got["result"].shape == want["result"].shape
    assert dist <= g_res
    for tr in ("rel_trace", "abs_trace"):
        a, b = np.array(got[tr]), np.array(want[tr])
        assert a.shape == b.shape == (want["n_cycles"],)
        assert np.all(np.abs(a - b) <= g_tr), (tr, a, b)
    assert got["lowest"] == min(got["rel_trace"])


def launch_names(nat, run):
    nat.prof_enable(True)
    nat.prof_collect()
    try:
        out = run()
        nat.prof_collect()
        return out, [n for n, _, _ in nat.prof_launch_log()]
    finally:
        nat.prof_enable(False)


# ----------------------------------------------------------------------------------------------------------------- 1
def test_defaults_keep_the_bits(dev):
    nat = pkg("_native")
    p = pair("hex13_dirichlet_s0", dev)
    eng = p.dp.eng
    plain, aug = eng.DeviceGmres64(p.dp.fmap, 10), handle(p, 10, 2)
    try:
        want, names_w = launch_names(nat, lambda: plain.solve_adjoint(p.hs, p.grad, EPS, 1500))
        got, names_g = launch_names(nat, lambda: aug.solve_adjoint(p.hs, p.grad, EPS, 1500, augment=0, stall=0.5))
        assert (got.pop("n_aug"), got.pop("augment")) == (0, 0)
        hr.same_out(got, want, "solve_adjoint, augment 0 stall 0.5 on a handle made with augment 2")
        assert names_g == names_w and len(names_w) > 100 and not any(n.startswith("k_lg64") for n in names_g)
        assert want["n_cycles"] >= 3 and want["n_reorth"] > 0
        assert aug.nbytes == plain.nbytes + 3 * p.grad.numel() * 8   # the ring: augment + 1 vectors
        q = lin("hex13_dirichlet_s0", dev)
        plain_s, aug_s = q.dp.eng.DeviceGmres64(q.dp.fmap, 8), handle(q, 8, 2)
        try:
            for shift, transposed in ((1.0, False), (1.5, True)):
                kw = dict(shift=shift, transposed=transposed, eta=1e-8, max_products=200)
                want, names_w = launch_names(nat, lambda: plain_s.solve_shifted(q.H, q.b, **kw))
                got, names_g = launch_names(nat, lambda: aug_s.solve_shifted(q.H, q.b, augment=0, stall=0.5, **kw))
                assert (got.pop("n_aug"), got.pop("augment")) == (0, 0)
                hr.same_out(got, want, f"solve_shifted shift {shift}")
                assert names_g == names_w and len(names_w) > 50
        finally:
            plain_s.close()
    finally:
        plain.close()
    # the Newton solver made through the new entry points, nothing kept, the plain rule
    fp = fixture_problem("hex13_dirichlet_s0", dev)
    x0 = fp.h0.to(dev)
    nt, nta = eng.DeviceNewton64(fp.fmap, 10), eng.DeviceNewton64Aug(fp.fmap, 10, augment=0)
    try:
        want, names_w = launch_names(nat, lambda: nt.solve(x0, eps=1e-11, threshold=12))
        got, names_g = launch_names(nat, lambda: nta.solve(x0, eps=1e-11, threshold=12, lin_stall=0.5))
        hr.same_out(got, want, "DeviceNewton64Aug(augment 0), lin_stall 0.5")
        assert names_g == names_w and want["n_products"] > 20
        assert nta.nbytes == nt.nbytes
    finally:
        nt.close()
        nta.close()


# ----------------------------------------------------------------------------------------------------------------- 2
def device_restatement(p, budget, m, augment, stall):
    key = (id(p), budget, m, augment, stall)
    if key not in _runs:
        op = lambda w: p.dp.fmap.vjp(p.hs, w)
        _runs[key] = lg.lgmres_adjoint(op, p.grad.double(), EPS, budget, m=m, augment=augment, stall=stall, device=p.dev)
    return _runs[key]


@pytest.mark.parametrize("augment", [1, 2])
@pytest.mark.parametrize("name", ref.FIXTURES)
def test_the_device_follows_the_restatement(name, augment, dev):
    p = pair(name, dev)
    want = device_restatement(p, 60, 10, augment, 1.0)
    got = handle(p, 10, 2).solve_adjoint(p.hs, p.grad, EPS, 60, augment=augment, stall=1.0)
    against_restatement(f"{name} m 10 augment {augment} budget 60", got, want, 2)
    assert got["augment"] == augment
    # the case is what it is meant to be: seven heads of a cycle; cycles 0 .. 4 are full with 0, 1, 2, .. stored corrections, cycle 5
    # has left = 4, so ka = augment, and the seventh head finds the budget spent
    assert (want["nstep"], want["n_cycles"], want["stop"]) == (60, 7, "budget")
    assert want["n_aug"] == sum(min(c, augment) for c in range(5)) + augment


# ----------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("name", ref.FIXTURES)
def test_it_converges_in_fewer_products(name, dev):
    p = pair(name, dev)
    h = handle(p, 10, 2)
    plain = h.solve_adjoint(p.hs, p.grad, EPS, 1500, augment=0, stall=0.5)
    runs = {a: h.solve_adjoint(p.hs, p.grad, EPS, 1500, augment=a, stall=1.0) for a in (0, 1, 2)}
    err = {a: p.ap.error(r["result"]) for a, r in runs.items()}
    print(f"LGM {name} m 10: stall 0.5 {plain['stop']} after {plain['nstep']} products, lowest {plain['lowest']:.3e}; stall 1.0, augment "
          + "; ".join(f"{a}: {r['stop']} after {r['nstep']} products ({r['n_cycles']} cycles, n_aug {r['n_aug']}), lowest "
                      f"{r['lowest']:.3e}, error {err[a]:.2e}" for a, r in runs.items()))
    if name in ("hex26_dirichlet_s0", "hex13_mixed_s1"):
        assert plain["stop"] == "stagnation" and plain["lowest"] > 1e-4
    for a, r in runs.items():
        assert r["stop"] == "tolerance" and r["lowest"] < EPS and r["nstep"] <= 1500
        assert (r["n_aug"] > 0) == (a > 0)
    for a in (1, 2):
        assert runs[a]["nstep"] < runs[0]["nstep"]
        assert err[a] <= 4.0 * err[0]


# ----------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("shift", [1.0, 1.5])
def test_shifted_system(shift, transposed, dev):
    q = lin("hex13_dirichlet_s0", dev)
    fm = q.dp.fmap
    op = (lambda v: fm.vjp(q.H, v)) if transposed else (lambda v: fm.jvp(q.H, v))
    want = lg.lgmres_adjoint(op, q.b, 1e-8, 200, m=8, augment=2, stall=1.0, shift=shift, lin=True, device=dev)
    got = handle(q, 8, 2).solve_shifted(q.H, q.b, shift=shift, transposed=transposed, eta=1e-8, max_products=200, stall=1.0)
    against_restatement(f"shifted, shift {shift} {'J^T' if transposed else 'J'} m 8 augment 2", got, want, 4)
    res = true_rel(fm, q.H, q.b, got["result"], shift, transposed)
    print(f"LGM shifted: lowest {got['lowest']:.6e} recomputed {res:.6e}")
    assert got["stop"] == "tolerance" and got["augment"] == 2
    np.testing.assert_allclose(res, got["lowest"], rtol=1e-6)
    assert res <= 1e-8


# ----------------------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("N", [1, 51, 52, 103, 129])
def test_smallest_shapes(N, dev):
    """M = 10 is below one block; 510 / 520 are either side of a 512-element block; 1 030 is across a 1 024 chunk; 1 290 is three
    blocks and two chunks."""
    p = Problem(vb.line_graph(N, False), load_weights("dirichlet"), dev)
    H = p.h0.to(dev)
    grad = torch.randn(H.shape, generator=torch.Generator().manual_seed(N), dtype=torch.float64).to(dev)
    op = lambda w: p.fmap.vjp(H, w)
    gm = p.eng.DeviceGmres64Aug(p.fmap, 4, 3)
    try:
        assert gm.nbytes >= (5 + 3 + 4) * H.numel() * 8
        lefts = set()
        for c in (1, 2, 3):
            for left in (1, 2):
                budget = 5 * c + 1 + left
                want = lg.lgmres_adjoint(op, grad, EPS, budget, m=4, augment=3, stall=1.0, device=dev)
                got = gm.solve_adjoint(H, grad, EPS, budget, stall=1.0)
                against_restatement(f"line{N} m 4 augment 3 budget {budget}", got, want, 5)
                if want["nstep"] == budget:   # every cycle was full: the last one had `left` steps, min(c, 3, left - 1) of them kept ones
                    lefts.add(left)
                    assert want["n_aug"] == sum(min(i, 3) for i in range(c)) + min(c, left - 1)
        assert lefts == {1, 2}   # both short last cycles were reached at this size
    finally:
        gm.close()


# ----------------------------------------------------------------------------------------------------------------- 6
def test_same_bits(dev):
    p = pair("hex13_dirichlet_s0", dev)
    run_b = lambda h: h.solve_adjoint(p.hs, p.grad, EPS, 200, augment=2, stall=1.0)
    run_a = lambda h: h.solve_adjoint(p.hs, 0.5 * p.grad, 1e-6, 45, augment=1, stall=0.9)   # another system, another ring
    chain = hr.Reused("gmres64 augmented", lambda: p.dp.eng.DeviceGmres64Aug(p.dp.fmap, 10, 2))
    try:
        first = chain.link("augment 2", run_b)
        assert first["n_aug"] > 0 and first["n_cycles"] > 4
        hr.same_out(run_b(chain.h), first, "twice on one handle")
        for pe in (1, 8, 1000):
            hr.same_out(chain.h.solve_adjoint(p.hs, p.grad, EPS, 200, poll_every=pe, augment=2, stall=1.0), first, f"poll_every {pe}")
        a = chain.link("half the gradient, augment 1", run_a)
        assert a["n_aug"] > 0
        hr.same_out(chain.link("augment 2 after A", run_b), first, "B after A against the first B: the ring is cleared")
        assert chain.pairs >= 2
    finally:
        chain.close()


# ----------------------------------------------------------------------------------------------------------------- 7
@pytest.mark.parametrize("name", ["hex13_dirichlet_s0", "hex13_mixed_s1"])
def test_newton_with_kept_corrections(name, dev):
    fp = fixture_problem(name, dev)
    nt = fp.eng.DeviceNewton64Aug(fp.fmap, m=10, augment=2)
    try:
        out = nt.solve(fp.h0.to(dev), lin_stall=1.0)
        assert nt.nbytes >= (11 + 3 + 6) * fp.h0.numel() * 8
    finally:
        nt.close()
    dist = rel_l2(out["result"], fp.golden["fp64_result"])
    f = fp.fmap(out["result"])
    rel = float((f - out["result"]).norm()) / (float(f.norm()) + 1e-9)
    print(f"LGM {name} Newton m 10 augment 2 lin_stall 1.0: stop {out['stop_reason']} n_iter {out['n_iter']} products {out['n_products']} "
          f"lowest {out['lowest']:.3e} recomputed {rel:.3e} distance to the stored fp64_result {dist:.2e} krylov {out['krylov']} "
          f"lin {sorted(set(out['lin_stop']))}")
    assert out["stop_reason"] == "tolerance" and out["lowest"] < 1e-11 and rel < 1e-11
    assert dist <= 5e-9


# ----------------------------------------------------------------------------------------------------------------- 8
def test_refusals_on_open_handles(dev):
    nat = pkg("_native")
    p = pair("hex13_dirichlet_s0", dev)
    eng, fm = p.dp.eng, p.dp.fmap
    gm = eng.DeviceGmres64Aug(fm, 10, 1)
    try:
        good = lambda: gm.solve_adjoint(p.hs, p.grad, EPS, 60, stall=1.0)
        before = good()
        assert before["augment"] == 1 and before["n_aug"] > 0
        with pytest.raises(nat.NativeError, match="augment must be in 0 .. 1"):
            gm.solve_adjoint(p.hs, p.grad, EPS, 60, augment=2)
        hr.same_out(good(), before, "after an augment above the handle's")
        for stall in (0.0, 1.5, float("nan")):
            with pytest.raises(nat.NativeError, match=r"stall must be in \(0, 1\]"):
                gm.solve_adjoint(p.hs, p.grad, EPS, 60, stall=stall)
            with pytest.raises(nat.NativeError, match=r"stall must be in \(0, 1\]"):
                gm.solve_shifted(p.hs, p.grad, stall=stall)
            hr.same_out(good(), before, f"after stall {stall}")
        for m, augment in ((10, 10), (4, 4), (20, 9)):
            with pytest.raises(nat.NativeError, match="augment must be in 0 .."):
                eng.DeviceGmres64Aug(fm, m, augment)
            with pytest.raises(nat.NativeError, match="augment must be in 0 .."):
                eng.DeviceNewton64Aug(fm, m, augment)
        hr.same_out(good(), before, "after the refused handles")
        # the C entry points say no with a code and a message, before any launch
        lib = nat.lib()
        h = ctypes.c_void_p()
        assert lib.psignn_gmres64_create_aug(ctypes.byref(h), fm.handle, 10, 10) < 0 and not h.value
        assert "augment out of range" in lib.psignn_last_error().decode()
        assert lib.psignn_newton64_create_aug(ctypes.byref(h), fm.handle, 10, 9) < 0 and not h.value
        need = lib.psignn_f64_deriv_workspace_doubles(fm.handle, 1, 1)
        work = torch.zeros(max(need, 1), dtype=torch.float64, device=dev)
        hs, gr = p.hs.double(), p.grad.double()
        out, info = torch.full_like(gr, 7.0), nat.Gmres64Info()
        args = lambda o: (gm.handle, nat.ptr(fm.wflat), 1, nat.ptr(hs), nat.ptr(fm.h0), nat.ptr(fm.prb), None, nat.ptr(gr), EPS, 60, 8,
                          ctypes.byref(o), nat.ptr(work), need, nat.ptr(out), info, None, None, None)
        for o, word in ((nat.Gmres64Opts(2, 1.0), "augment"), (nat.Gmres64Opts(1, 0.0), "stall"), (nat.Gmres64Opts(1, 1.5), "stall"),
                        (nat.Gmres64Opts(1, math.nan), "stall"), (nat.Gmres64Opts(-1, 0.5), "augment")):
            assert lib.psignn_gmres64_solve_adjoint_opts(*args(o)) < 0
            assert word in lib.psignn_last_error().decode()
        torch.cuda.synchronize(dev)
        assert bool((out == 7.0).all())   # nothing was written
        assert lib.psignn_gmres64_solve_adjoint_opts(*args(nat.Gmres64Opts(1, 1.0))) == 0
        assert (info.products, info.cycles, info.n_aug) == (before["nstep"], before["n_cycles"], before["n_aug"])
        assert hr.same_tensor(out, before["result"])
        hr.same_out(good(), before, "after the refused native calls")
    finally:
        gm.close()
    with pytest.raises(nat.NativeError, match="closed"):
        gm.solve_adjoint(p.hs, p.grad, EPS, 60)
    # the convenience
    md = p.ap.mesh.to(dev)
    got = eng.adjoint64_aug(md, p.ap.sd, p.hs, p.grad, eps=EPS, m=10, max_products=60, augment=1, stall=1.0)
    hr.same_out(got, before, "adjoint64_aug")
