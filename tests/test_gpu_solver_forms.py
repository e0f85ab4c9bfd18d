"""Every form of the on-device Broyden update, in every regime, against the reference's recurrences.

csrc/solver.hip runs the rank-one update of ``broyden`` (utilities/solver.py:185-192) in several forms chosen by vector
length and by the number k of stored pairs: two passes over U and V (short vectors), three single-array sweeps U, V, U, the
third sweep folded with the next iteration's first one while k <= 24 (kept values in registers, ``k_sweep_u2r<KB>``, or in
per-thread LDS slots, ``k_sweep_u2d``), and beyond that a WINDOW of the 16 most recent pairs kept plus a partial first sweep
over the older ones -- the regime every real solve (``fw_thres`` 500 - 1 500) spends almost all its iterations in.

A Broyden trajectory cannot pin these forms against the CPU oracle over 48 iterations: measured on the oracle itself
(f(x) = c * x + b, fp32), a relative perturbation of 1e-7 of the start moves ``rel_trace`` by O(1) from iteration ~18 on -- every
update divides by vT . dg, a difference of nearly equal numbers.  What CAN be checked exactly, at any k, is each iteration by
itself: the solver's own state (iterates, update vectors, stored pairs U_j, V_j, read back through
``psignn_broyden_get_iterate / _get_pair``) must satisfy

    vT     = -dx + sum_j (U_j . dx) V_j                                  (rmatvec, solver.py:96-104, 186)
    u      = (dx + dg - sum_j (V_j . dg) U_j) / (vT . dg)                (matvec, solver.py:106-114, 187)
    update = g - sum_{j<=k} (V_j . g) U_j                                (solver.py:192)

evaluated in float64 ON THE CPU from the device's previous state.  The tolerance is not fitted: a device quantity may be at
most 16 x as far from the float64 value as a plain float32 evaluation of the same formula (torch CPU, other summation order) is.
A missed pair, a wrong coefficient, a stale `a`, an uncovered element range are off by a factor 1e4 or more on this scale.
Besides: the first iterations against ``oracle.broyden`` (before the chaos), the converged iterate against the closed form
b / (1 - c), bit-equality of the register and LDS forms of the folded sweep, and bit-equality of batched, fused single-mesh
and host-driven solves, which carries the check over to ``psignn_broyden_solve`` and ``psignn_broyden_solve_batch``."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_weights, pkg, rel_l2
from oracle import psignn_oracle as orc
# K = 48 iterations per solve: the window regime starts at k = 25 with the default limits
from recurrences import K, _check_run, _Recorder, _run_recorded   # noqa: F401  (test_gpu_broyden_bf16.py takes _Recorder from here)

pytestmark = pytest.mark.gpu

ENVS = {
    "default": {},                                                  # fold in registers on long vectors / big shards, in LDS below; all pairs kept to k = 24, then a window of 16
    "reg": {"PSIGNN_U2D_FORM": "reg"},                              # k_sweep_u2r<KB>
    "lds": {"PSIGNN_U2D_FORM": "lds"},                              # k_sweep_u2d: round-2 form of the same fold
    "keep8": {"PSIGNN_U2D_FORM": "reg", "PSIGNN_U2D_KEEP": "8"},    # window of 8: k_sweep_u2r<8> in the window regime
    "window_from_5": {"PSIGNN_U2D_FORM": "reg", "PSIGNN_U2D_KMAX": "4", "PSIGNN_U2D_KEEP": "2"},
    "no_fold": {"PSIGNN_U2D_KMAX": "0"},                            # plain three-sweep form
    "two_pass": {"PSIGNN_UVU": "0"},                                # dots + axpy + final
    "lds_max": {"PSIGNN_U2D_FORM": "lds", "PSIGNN_U2D_KMAX": "31", "PSIGNN_U2D_KEEP": "31"},   # LDS fold at its limit: 32 partials = PARTA_LD
}
_KNOBS = ("PSIGNN_U2D_FORM", "PSIGNN_U2D_KEEP", "PSIGNN_U2D_KMAX", "PSIGNN_UVU", "PSIGNN_JGROUPS")


def _setenv(monkeypatch, env):
    for k in _KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _linear(N, cmax, dev, seed=0):
    gen = torch.Generator().manual_seed(seed)
    c = 0.05 + (cmax - 0.05) * torch.rand(N, 10, generator=gen)
    b = torch.randn(N, 10, generator=gen)
    x0 = torch.randn(N, 10, generator=gen)
    return c, b, x0


ITS = (0, 1, 4, 5, 7, 9, 16, 17, 23, 24, 25, 26, 33, 40, 46)      # default form
ITS_SHORT = (1, 5, 6, 24, 25, 26, 46)                             # the other forms: window entry (k = 5 / 25), both sides of it


SIZES = {"mid": (100000, False), "long": (100000, True), "ragged": (100001, False), "ragged_long": (100001, True)}


@pytest.mark.parametrize("size", list(SIZES))
def test_update_forms_satisfy_the_broyden_recurrences(size, dev, monkeypatch):
    """f(x) = c * x + b on (100 000, 10) through the generic-callable path (``psignn_broyden_ext_*``; M = 1 M elements).
    "mid": the natural shapes at this length (4 floats per lane, unsplit sweeps: the form of 100k-node meshes and of batched
    shards); "long": PSIGNN_JGROUPS=1 selects the long-vector shapes (16 floats per lane: the form of the 1M-node headline).
    "ragged" / "ragged_long": the same on (100 001, 10), M = 1 000 010 = 10 (mod 16): a ragged quad in the register fold
    ``k_sweep_u2r`` and a ragged lane in the 16-float three-sweep form (every check also runs on the last 4 096 elements).
    Each variant of the update: recurrences at iterations spanning the all-kept regime, the transition k = 24 -> 25 and the
    window regime; first iterations vs the CPU oracle; register and LDS forms of the fold bit-identical."""
    eng = pkg("engine")
    N, jg = SIZES[size]
    c, b, x0 = _linear(N, 0.995, dev)
    cd, bd, x0d = c.to(dev), b.to(dev), x0.to(dev)
    f = lambda x: cd * x + bd
    with torch.no_grad():
        ref = orc.broyden(lambda x: c * x + b, x0, threshold=10, eps=0.0)
    base = {"PSIGNN_JGROUPS": "1"} if jg else {}
    outs = {}
    for name, env in ENVS.items():
        _setenv(monkeypatch, {**base, **env})
        rec, sv, out = _run_recorded(eng, f, x0d, n_elems=x0d.numel())
        np.testing.assert_allclose(out["rel_trace"][:8], ref["rel_trace"][:8], rtol=1e-3, err_msg=name)
        # (the oracle's float32 einsum over 1 M elements is the less accurate side here: its dot products carry ~1e-5)
        assert rel_l2(rec.X[3], ref["xest_trace"][3]) < 1e-5 and rel_l2(rec.X[6], ref["xest_trace"][6]) < 5e-4, name
        _check_run(rec, sv, ITS if name == "reg" else ITS_SHORT, f"{size}/{name}")
        outs[name] = (out, [rec.X[i] for i in (10, 30, K)])
        sv.close()
    _setenv(monkeypatch, {})
    # kept values in registers or in LDS: same operations in the same order, same partial-sum shapes
    (a, xa), (l, xl) = outs["reg"], outs["lds"]
    assert a["rel_trace"] == l["rel_trace"] and all(torch.equal(p, q) for p, q in zip(xa, xl))
    d, xd = outs["default"]                                          # the default is one of the two
    assert d["rel_trace"] == a["rel_trace"] and all(torch.equal(p, q) for p, q in zip(xd, xa))
    # every form is the same iteration up to rounding: the early trace agrees closely, the residual keeps falling in all of them
    for name, (o, _) in outs.items():
        np.testing.assert_allclose(o["rel_trace"][:10], a["rel_trace"][:10], rtol=2e-3, err_msg=name)
        assert o["lowest"] < 0.5 * o["rel_trace"][9], (name, o["lowest"], o["rel_trace"][9])   # (not monotone: rank-one updates spike)


def test_long_vector_natural_size_and_closed_form(dev, monkeypatch):
    """(320 000, 10) = 3.2 M elements: the long-vector form without any knob (16 floats per lane, fold in registers, window
    from k = 25).  Recurrences in the window regime; and a well-conditioned problem (c <= 0.5) converges, in every form, to
    the closed-form fixed point b / (1 - c) (48 iterations, most of them at the rounding floor with vT.dg ~ 0 -- NaN / inf
    scrubbing of solver.py:188-189 included)."""
    eng, solver = pkg("engine"), pkg("utilities.solver")
    _setenv(monkeypatch, {})
    c, b, x0 = _linear(320000, 0.995, dev, seed=1)
    cd, bd, x0d = c.to(dev), b.to(dev), x0.to(dev)
    rec, sv, out = _run_recorded(eng, lambda x: cd * x + bd, x0d, n_elems=x0d.numel())
    _check_run(rec, sv, (23, 24, 25, 31, 46), "3.2M/default")
    sv.close()
    del rec
    c, b, x0 = _linear(320000, 0.5, dev, seed=2)
    cd, bd, x0d = c.to(dev), b.to(dev), x0.to(dev)
    xstar = b / (1 - c)
    for name, env in ENVS.items():
        _setenv(monkeypatch, env)
        o = solver.broyden(lambda x: cd * x + bd, x0d, threshold=K, eps=0.0, keep_trace=False)
        assert rel_l2(o["result"], xstar) < 1e-6, (name, rel_l2(o["result"], xstar))
        assert o["lowest"] < 2e-7 and bool(torch.isfinite(o["result"]).all()), (name, o["lowest"])
    _setenv(monkeypatch, {})


@pytest.mark.parametrize("N", [1, 25, 409])
def test_update_on_vectors_shorter_than_a_block(N, dev, monkeypatch):
    """M = 10 (one node: less than a quad of lanes), 250 (less than one wave), 4 090 (a partial last block, M % 4 = 2) through
    the generic-callable path: the first iterations against the CPU oracle, the recurrences while k is well below M; and a
    well-conditioned problem converges to the closed form b / (1 - c) and stays finite through 48 iterations -- more than M
    for the first two, so the iteration spends its last ones at the rounding floor with vT.dg ~ 0 (the NaN / inf scrubbing of
    solver.py:188-189)."""
    eng, solver = pkg("engine"), pkg("utilities.solver")
    _setenv(monkeypatch, {})
    M = N * 10
    c, b, x0 = _linear(N, 0.995, dev, seed=3)
    cd, bd, x0d = c.to(dev), b.to(dev), x0.to(dev)
    with torch.no_grad():
        ref = orc.broyden(lambda x: c * x + b, x0, threshold=6, eps=0.0)
    rec, sv, out = _run_recorded(eng, lambda x: cd * x + bd, x0d, n_elems=M)
    np.testing.assert_allclose(out["rel_trace"][:4], ref["rel_trace"][:4], rtol=1e-3)
    assert rel_l2(rec.X[3], ref["xest_trace"][3]) < 1e-5
    _check_run(rec, sv, [i for i in (0, 1, 2, 3, 5, 9, 16, 24, 25, 26) if i <= M // 3], f"M={M}")
    sv.close()
    c, b, x0 = _linear(N, 0.5, dev, seed=4)
    cd, bd, x0d = c.to(dev), b.to(dev), x0.to(dev)
    o = solver.broyden(lambda x: cd * x + bd, x0d, threshold=K, eps=0.0, keep_trace=False)
    # once g is exactly 0, vT.dg = 0 and u = D1 / 0 is inf, which the reference's scrubbing (x != x) leaves in place: its trace
    # turns NaN from there on too (oracle.broyden on this problem at M = 4 090) -- but only after the iteration has converged,
    # and the result (the lowest iterate) stays finite
    tr = o["rel_trace"]
    bad = next((i for i, v in enumerate(tr) if not np.isfinite(v)), len(tr))
    assert bool(torch.isfinite(o["result"]).all()) and bad > 0 and min(tr[:bad]) < 2e-7, (M, bad, tr[:bad])
    assert rel_l2(o["result"], b / (1 - c)) < 1e-6 and o["lowest"] < 2e-7, (M, rel_l2(o["result"], b / (1 - c)), o["lowest"])


def _first_launch_iteration(log, name):
    """Iteration (0-based) of the first launch of `name` in a launch log of one solve: one k_reduce_check per iteration,
    launched before sweeps 2 and 3 of that iteration and after its sweep 1."""
    it = 0
    for n, _, _ in log:
        if n == name:
            return it
        it += n == "k_reduce_check"
    return None


def test_lds_fold_keeps_at_most_a_row_of_partials(dev, monkeypatch):
    """The LDS form of the folded sweep keeps at most PARTA_LD = 32 partials per row (pairs keep0 .. k): PSIGNN_U2D_KMAX /
    _KEEP are capped at 31 there.  Asked for 38 / 36, the library used to keep up to 39 pairs and drop the partials past the
    row pitch, and the next iteration read the neighbouring block's row in their place (wrong a_32 ... a_38, no fault).

    At the limit (31 / 31) the fold supplies every a_j through iteration 32 (at 32 it keeps pairs 1 .. 32: exactly one row),
    so the first sweep 1 runs in iteration 33 -- not earlier (a cap of 15, the fallback when the LDS attribute is refused,
    would show here); the recurrences hold on both sides; a request of 38 / 36 is the same solve, bit for bit."""
    eng, nat = pkg("engine"), pkg("_native")
    c, b, x0 = _linear(100000, 0.995, dev, seed=5)
    cd, bd, x0d = c.to(dev), b.to(dev), x0.to(dev)
    f = lambda x: cd * x + bd
    M = x0d.numel()
    runs = {}
    for name, env in (("lds_max", ENVS["lds_max"]), ("ask_38", {"PSIGNN_U2D_FORM": "lds", "PSIGNN_U2D_KMAX": "38", "PSIGNN_U2D_KEEP": "36"})):
        _setenv(monkeypatch, env)
        nat.prof_enable(True)
        nat.prof_collect()
        try:
            rec, sv, out = _run_recorded(eng, f, x0d, n_elems=M)
            nat.prof_collect(with_bytes=True)
            log = nat.prof_launch_log()
        finally:
            nat.prof_enable(False)
        assert _first_launch_iteration(log, "k_sweep_u1") == 33, (name, _first_launch_iteration(log, "k_sweep_u1"))
        it = -1
        for n, _, byts in log:       # the fold's stated bytes: k columns of U + update, dg, g, U_k, update (per iteration k)
            it += n == "k_reduce_check"
            if n == "k_sweep_u2d":
                assert byts == (it + 5) * M * 4, (name, it, byts)
        if name == "lds_max":
            _check_run(rec, sv, (30, 31, 32, 33, 40, 46), "lds_max")
        runs[name] = (out["rel_trace"], [rec.X[i] for i in (10, 32, 33, 34, 40, K)])
        sv.close()
        del rec
    _setenv(monkeypatch, {})
    (ra, xa), (rb, xb) = runs["lds_max"], runs["ask_38"]
    assert ra == rb and all(torch.equal(p, q) for p, q in zip(xa, xb))


_CHAIN = {"k_sweep_u1", "k_sweep_v", "k_sweep_u2", "k_sweep_u2d", "k_reduce_check", "k_reduce_cb", "k_dots", "k_axpy", "k_axpy_combine", "k_final"}


@pytest.fixture(scope="module")
def schedule_table():
    with open(os.path.join(GOLDEN, "broyden_schedule.json")) as f:
        return {r["case"]: r for r in json.load(f)}


@pytest.mark.parametrize("case", ["m4090", "width_switch", "above_reg_fold"])
def test_library_runs_the_recorded_schedule(case, schedule_table, dev, monkeypatch):
    """The built library against rows of tests/golden/broyden_schedule.json -- the table csrc/solver_shapes.h is checked against on
    the CPU (tests/test_host_solver_shapes.py): ``nbytes`` of the handle and, per iteration of a solve with eps = 0, the update
    chain's launches with their stated bytes.  M = 4 090: two-pass form, 4 floats per lane, a partial last block, the split and
    its combine launch from k = 32.  M = 3 << 18, 28 iterations: the three-sweep form at the width switch, the fold crossing
    k = 24 into the window.  M = 2 047 * 1 024 + 1, the shortest vector with the fold in registers: KB = 8 / 16 / 24 all occur."""
    eng, nat = pkg("engine"), pkg("_native")
    row = schedule_table[case]
    M, thr = row["M"], row["thr"]
    assert row["env"] == {} and row["n_tiles"] == 0 and row["hist"] == 0
    _setenv(monkeypatch, {})
    monkeypatch.delenv("PSIGNN_VEC16_MIN", raising=False)
    monkeypatch.delenv("PSIGNN_VEC_AX4", raising=False)
    gen = torch.Generator().manual_seed(0)
    seq = 10 if M % 10 == 0 else 1                 # (as the table was recorded)
    shape = (M // seq, seq)
    c, b, x0 = (t.to(dev) for t in (0.05 + 0.945 * torch.rand(shape, generator=gen), torch.randn(shape, generator=gen), torch.randn(shape, generator=gen)))
    sv = eng.DeviceBroyden(threshold=thr, keep_trace=bool(row["keep_trace"]), n_elems=M, seq_len=seq, device=dev)
    assert sv.nbytes == row["nbytes"]
    nat.prof_enable(True)
    nat.prof_collect()
    try:
        out = sv.solve_callable(lambda x: c * x + b, x0, 0.0)
        nat.prof_collect(with_bytes=True)
        log = nat.prof_launch_log()
    finally:
        nat.prof_enable(False)
    sv.close()
    assert out["n_iter"] == thr
    iters = []
    for name, _, byts in log:
        if name == "k_resid":                      # the head of every iteration of a host-driven solve
            iters.append([])
        elif name in _CHAIN:
            assert byts % M == 0, (name, byts)
            iters[-1].append([name, byts // M])
    assert iters == row["iters"]
    if case == "above_reg_fold":                   # kept pairs k - keep0: 0 .. 24 while all are kept, then the window of 16
        assert sum(n == "k_sweep_u2d" for it in iters for n, _ in it) == thr - 1


def _mesh_map(n, seed, dev, sd, phase=0.0):
    data, eng = pkg("data"), pkg("engine")
    mesh = data.make_hex_problem(n, seed=seed, compute_sol=False, phase=phase)
    md = mesh.to(dev)
    with torch.no_grad():
        h0 = orc.encoder(sd, mesh.x)
    plan = eng.MeshPlan(md)
    return eng.FixedPointMap(plan, eng.PackedWeights(sd, dev), h0.to(dev), md.prb_data, None)


def test_fused_device_solve_is_the_host_driven_solve(dev, monkeypatch):
    """``psignn_broyden_solve`` (f fused with x + update, g, dg and the norm partials; everything on the device) against the
    host-driven solve of the same map through ``psignn_broyden_ext_*`` on a 99 919-node mesh, 48 iterations: the two share
    launch_update, so every iterate is bit-identical -- which carries the recurrence check of the host-driven run (GNN map,
    window regime included) over to the fused solver."""
    eng, solver = pkg("engine"), pkg("utilities.solver")
    _setenv(monkeypatch, {})
    fm = _mesh_map(182, 0, dev, load_weights("dirichlet"))
    assert fm.plan.tiled and fm.plan.N == 99919
    rec, sv, out = _run_recorded(eng, fm.fp, fm.to_plan(fm.h0), plan=fm.plan, back=fm.from_plan)
    rec.fwd = fm.to_plan
    _check_run(rec, sv, (3, 12, 24, 25, 26, 40, 46), "gnn 100k")
    fused = solver.broyden(fm, fm.h0, threshold=K, eps=0.0, keep_trace=True)
    assert fused["n_iter"] == K
    for i in (1, 9, 24, 25, 26, 40, K):
        assert torch.equal(fused["xest_trace"][i], rec.X[i]), i
    np.testing.assert_allclose(fused["rel_trace"][:K], out["rel_trace"][:K], rtol=1e-5)   # (norm partials: per tile vs per block)
    sv.close()


@pytest.mark.parametrize("envname", ["reg", "lds", "window_from_5", "lds_max", "no_fold", "two_pass"])
def test_batched_shard_in_the_window_regime(envname, dev, monkeypatch):
    """``psignn_broyden_solve_batch`` through 48 iterations (window regime from k = 25; from k = 5 with the small limits) on a
    shard of 8 x 10 267-node meshes -- the shapes of BASELINE configs[3] (shard-sized reductions, 4 floats per lane): every mesh
    bit-identical to its own fused solve with the same solver object, that one bit-identical to the host-driven solve, and the
    host-driven solve satisfies the recurrences.  ``no_fold`` / ``two_pass``: the shard's plain sweep 3 and its two-pass form with
    the axpy pass at its own width."""
    eng = pkg("engine")
    _setenv(monkeypatch, ENVS[envname])
    sd = load_weights("dirichlet")
    fms = [_mesh_map(58, s, dev, sd, phase=0.37 * s) for s in range(8)]
    w0 = fms[0].weights
    for f in fms[1:]:
        f.weights = w0                                             # one packed weight buffer for the shard
    total = sum(f.plan.N for f in fms) * 10
    solvers = [eng.DeviceBroyden(plan=f.plan, threshold=K, keep_trace=True, shard_elems=total) for f in fms]
    outs = eng.broyden_solve_batch(solvers, fms, 0.0)
    its_b = [[sv.iterate(i, f.h0) for i in (1, 24, 25, 26, 40, K)] for sv, f in zip(solvers, fms)]
    for m in (0, 5):
        single = solvers[m].solve(fms[m], 0.0)
        assert single["rel_trace"] == outs[m]["rel_trace"] and torch.equal(single["result"], outs[m]["result"])
        assert all(torch.equal(solvers[m].iterate(i, fms[m].h0), x) for i, x in zip((1, 24, 25, 26, 40, K), its_b[m]))
    for sv in solvers:
        sv.close()
    fm = fms[5]
    rec, sv, out = _run_recorded(eng, fm.fp, fm.to_plan(fm.h0), plan=fm.plan, shard_elems=total, back=fm.from_plan)
    rec.fwd = fm.to_plan
    for i, x in zip((1, 24, 25, 26, 40, K), its_b[5]):
        assert torch.equal(rec.X[i], x), i
    _check_run(rec, sv, (4, 5, 6, 24, 25, 26, 46), f"shard/{envname}")
    sv.close()
    _setenv(monkeypatch, {})


def test_batched_shard_at_the_narrow_width_splits_the_axpy_pass(dev, monkeypatch):
    """A ragged shard of three small meshes (together below 768 Ki elements: 4 floats per lane, two-pass form, sweeps split over
    8 groups of stored pairs), 48 iterations: from k = 4 * 8 = 32 on the shard runs the split axpy pass and its combine launch.
    Every mesh bit-identical -- result, iterates on both sides of k = 32, ``rel_trace`` -- to its own fused solve on the same
    solver object."""
    eng, nat = pkg("engine"), pkg("_native")
    _setenv(monkeypatch, {})
    sd = load_weights("dirichlet")
    fms = [_mesh_map(n, s, dev, sd, phase=0.37 * s) for s, n in enumerate((26, 34, 30))]
    for f in fms[1:]:
        f.weights = fms[0].weights                                 # one packed weight buffer for the shard
    total = sum(f.plan.N for f in fms) * 10
    assert total < 768 * 1024 and len({f.plan.N for f in fms}) == 3 and all(f.plan.tiled for f in fms)
    solvers = [eng.DeviceBroyden(plan=f.plan, threshold=K, keep_trace=True, shard_elems=total) for f in fms]
    assert eng.shard_batchable(solvers)
    nat.prof_enable(True)
    nat.prof_collect()
    outs = eng.broyden_solve_batch(solvers, fms, 0.0)
    ran = nat.prof_collect()
    nat.prof_enable(False)
    assert "k_dots" in ran and "k_sweep_v" not in ran, sorted(ran)     # the two-pass form ...
    assert ran["k_axpy_combine"][0] == K - 8 and ran["k_axpy"][0] == K, ran   # ... and the combine, launched from k = 8 on (it works from k = 32)
    its = (1, 31, 32, 33, K)
    its_b = [[sv.iterate(i, f.h0) for i in its] for sv, f in zip(solvers, fms)]
    for m, (sv, fm) in enumerate(zip(solvers, fms)):
        assert outs[m]["n_iter"] == K
        nat.prof_collect()
        nat.prof_enable(True)
        single = sv.solve(fm, 0.0)
        ran1 = nat.prof_collect()
        nat.prof_enable(False)
        assert ran1["k_axpy_combine"][0] == K - 32, ran1              # the mesh's own solve splits from k = 32: jgroups = 8
        assert single["rel_trace"] == outs[m]["rel_trace"] and torch.equal(single["result"], outs[m]["result"]), m
        assert all(torch.equal(sv.iterate(i, fm.h0), x) for i, x in zip(its, its_b[m])), m
        sv.close()
