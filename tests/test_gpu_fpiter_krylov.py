"""Picard and Anderson (csrc/fpiter.hip) and the device GMRES (csrc/krylov.hip) step by step against float64, at lengths that
reach every edge of the thread -> element mapping of the vector kernels, at both widths (4 floats per lane below 786 432
elements, 16 from there on).

The float64 step checkers live in tests/recurrences.py (and are themselves tested without a GPU in
tests/test_recurrence_checkers.py): every step is recomputed on the CPU from the device's own previous state, recorded by
wrapping f; each check also runs on the last 4 096 elements alone.  The map is f(x) = c * x + s * roll(x, 7) + b
(|c| + |s| < 1: a contraction that couples elements 7 apart, so the problem is not diagonal), or c * tanh(x) + b."""
import numpy as np
import pytest
import torch

import recurrences as rc
from conftest import pkg, rel_l2
from oracle import psignn_oracle as orc

pytestmark = pytest.mark.gpu

VEC16_FROM = 3 << 18      # psignn_fpiter_create / psignn_gmres_create: 16 floats per lane from 786 432 elements
LENGTHS = {
    10: "one node: less than a quad of lanes",
    250: "less than one wave",
    4090: "partial last block, M % 4 = 2 (4 floats per lane)",
    786430: "just below the width switch: 4 floats, M % 4 = 2",
    786440: "just above it: 16 floats, M % 16 = 8",
    1000010: "16 floats, M % 16 = 10, partial last block of 4 096",
}
FP_KERNELS = ("k_and_gram", "k_and_solve", "k_and_mix", "k_fp_norms", "k_and_check")


def _problem(M, dev, seed=0, rho=0.9, nonlinear=False, cpu64=False):
    """(f on the device, the same f on the CPU -- in float64 with ``cpu64`` --, x0 on the CPU), shape (M / 10, 10)."""
    N = M // 10
    gen = torch.Generator().manual_seed(seed)
    c = 0.05 + (rho - 0.25) * torch.rand(N, 10, generator=gen)
    s = 0.4 * (torch.rand(N, 10, generator=gen) - 0.5)
    b = torch.randn(N, 10, generator=gen)
    x0 = torch.randn(N, 10, generator=gen)
    cd, sd, bd = c.to(dev), s.to(dev), b.to(dev)
    if cpu64:
        c, s, b = c.double(), s.double(), b.double()
    if nonlinear:
        return (lambda x: cd * torch.tanh(x) + bd), (lambda x: c * torch.tanh(x) + b), x0
    return (lambda x: cd * x + sd * torch.roll(x, 7) + bd), (lambda x: c * x + s * torch.roll(x, 7) + b), x0


def _profiled(fn):
    nat = pkg("_native")
    nat.prof_enable(True)
    nat.prof_collect()
    try:
        out = fn()
        ran = nat.prof_collect()
    finally:
        nat.prof_enable(False)
    return out, ran


# ---------------------------------------------------------------------------------------------------------- Anderson
@pytest.mark.parametrize("M", [4090, 786440, 1000010])
def test_anderson_every_step_at_both_widths(M, dev):
    """m in {2, 3, 5, 8} (FP_MAX_M = 8: 36 Gram accumulators, the float4 walk over a 16-float span in k_and_gram), beta in
    {1, 0.6} (the X half of k_and_mix), 12 steps each (the ring wraps: slot k % m), every step against the float64 mix of the
    device's own ring slots; traces, result and nstep.  4 090: the mildly nonlinear map."""
    solver = pkg("utilities.solver")
    T = 14
    fg, _, x0 = _problem(M, dev, seed=1, rho=0.95, nonlinear=M < VEC16_FROM)
    x0d = x0.to(dev)
    for m in (2, 3, 5, 8):
        for beta in (1.0, 0.6):
            rec = rc.Recorder(fg)
            out, ran = _profiled(lambda: solver.anderson(rec, x0d, m=m, lam=1e-4, threshold=T, eps=0.0, beta=beta,
                                                         keep_trace=False))
            for name in FP_KERNELS:
                assert ran.get(name, (0,))[0] == T - 2, (M, m, beta, name, ran.get(name))
            rc.check_anderson(rec.P, rec.R, out, m, 1e-4, beta, T, 0.0, where=f"M={M} m={m} beta={beta}")


@pytest.mark.parametrize("M", list(LENGTHS))
def test_anderson_and_picard_at_every_length(M, dev):
    """Every length of the table: Anderson (m = 2, beta = 1: the reference's setting; m = 5, beta = 0.6) step by step and its
    first steps against ``oracle.anderson``; Picard step by step, its stop at the first rel <= eps and its result, and the
    trace against ``oracle.forward_iteration`` (the same fp32 map on both sides: the iterates are the same bits)."""
    solver = pkg("utilities.solver")
    fg, fc, x0 = _problem(M, dev, seed=2, rho=0.9, cpu64=True)
    x0d = x0.to(dev)
    T = 12
    for m, beta in ((2, 1.0), (5, 0.6)):
        rec = rc.Recorder(fg)
        out = solver.anderson(rec, x0d, m=m, lam=1e-4, threshold=T, eps=0.0, beta=beta, keep_trace=False)
        rc.check_anderson(rec.P, rec.R, out, m, 1e-4, beta, T, 0.0, where=f"M={M} m={m} beta={beta}")
        # (the oracle in float64: its float32 bmm over ~1 M elements carries ~1e-5 in the Gram matrix, which the bordered solve
        # of m = 5 amplifies to 2 % in the third residual -- the float32 oracle is the less accurate side there)
        ref_rec = rc.Recorder(fc)
        with torch.no_grad():
            ref = orc.anderson(ref_rec, x0.double(), m=m, lam=1e-4, threshold=6, eps=0.0, beta=beta)
        np.testing.assert_allclose(out["rel_trace"][:3], ref["rel_trace"][:3], rtol=1e-3, err_msg=f"M={M} m={m}")
        for k in (2, 3, 4):
            assert rel_l2(rec.P[k], ref_rec.P[k]) < 1e-5, (M, m, k, rel_l2(rec.P[k], ref_rec.P[k]))
    fg, fc, x0 = _problem(M, dev, seed=3, rho=0.6, nonlinear=M == 4090)
    rec = rc.Recorder(fg)
    out, ran = _profiled(lambda: solver.forward_iteration(rec, x0.to(dev), eps=1e-5, threshold=60))
    n = rc.check_picard(rec.P, rec.R, out, 60, 1e-5, where=f"picard M={M}")
    assert n < 61, (M, n)                                     # stopped on the tolerance
    assert ran["k_fp_norms"][0] == ran["k_picard_check"][0] == len(rec.P), (ran, len(rec.P))   # one per evaluation handed in
    with torch.no_grad():
        ref = orc.forward_iteration(fc, x0, eps=1e-5, threshold=60)
    assert abs(out["nstep"] - ref["nstep"]) <= 1, (out["nstep"], ref["nstep"])
    np.testing.assert_allclose([float(r) for r in out["rel_trace"][:5]], [float(r) for r in ref["rel_trace"][:5]], rtol=1e-4)


def test_anderson_abs_mode_early_stop(dev):
    """stop_mode="abs" at 786 440 elements (16 floats per lane), a tolerance met early, polled every 8 steps (the host runs
    ahead of the stop): every step up to the stop, result = the iterate of lowest |f(x) - x|, traces padded as the reference."""
    solver = pkg("utilities.solver")
    M, T = 786440, 40
    fg, _, x0 = _problem(M, dev, seed=4, rho=0.6)
    x0d = x0.to(dev)
    eps = 1e-4 * float((fg(x0d) - x0d).norm())
    rec = rc.Recorder(fg)
    out = solver.anderson(rec, x0d, m=3, lam=1e-4, threshold=T, eps=eps, stop_mode="abs", keep_trace=False, poll_every=8)
    n = rc.check_anderson(rec.P, rec.R, out, 3, 1e-4, 1.0, T, eps, stop_mode="abs", where="abs mode")
    assert n < T - 2, n


def test_anderson_history_length_outside_2_to_8_is_refused(dev):
    """m = 1 (no history to mix) and m = 9 (> FP_MAX_M) raise NativeError before anything is launched on them; the library
    works on afterwards."""
    solver, nat = pkg("utilities.solver"), pkg("_native")
    fg, _, x0 = _problem(4090, dev)
    x0d = x0.to(dev)
    for m in (1, 9):
        with pytest.raises(nat.NativeError):
            solver.anderson(fg, x0d, m=m, threshold=10, eps=0.0)
    out = solver.anderson(fg, x0d, m=2, threshold=10, eps=0.0)
    assert bool(torch.isfinite(out["result"]).all()) and out["lowest"] < out["rel_trace"][0]


# ---------------------------------------------------------------------------------------------------------- GMRES
def _gmres(M, dev, m_max, eta, seed=5, rho=0.9, zero_rhs=False):
    """DeviceGmres on A = J - I, J v = c * v + s * roll(v, 7) applied by torch on the device (the raw product goes into basis
    slot j + 1, shift 1, as newton_krylov does).  Returns (solver, steps done, float64 A on the CPU, b on the device)."""
    eng = pkg("engine")
    gen = torch.Generator().manual_seed(seed)
    c = 0.05 + (rho - 0.25) * torch.rand(M, generator=gen)
    s = 0.4 * (torch.rand(M, generator=gen) - 0.5)
    b = torch.zeros(M) if zero_rhs else torch.randn(M, generator=gen)
    cd, sd, bd = c.to(dev), s.to(dev), b.to(dev)
    c64, s64 = c.double(), s.double()
    gm = eng.DeviceGmres(M, dev, m_max)
    gm.begin(bd)
    k = 0
    for j in range(m_max):
        v = gm.row(j, (M,))
        gm.row(j + 1, (M,)).copy_(cd * v + sd * torch.roll(v, 7))
        k = j + 1
        if gm.step(j, 1.0, eta, poll=True):
            break
    return gm, k, (lambda v: c64 * v + s64 * torch.roll(v, 7) - v), bd


@pytest.mark.parametrize("reorth", ["default", "always"])
@pytest.mark.parametrize("M", [786430, 786440, 1000010])
def test_gmres_every_step_at_both_widths(M, reorth, dev, knobs):
    """20 Arnoldi steps (eta = 0: no early stop), conditional (default) or unconditional (PSIGNN_GMRES_REORTH=always) second
    Gram-Schmidt pass: the basis is orthonormal and A v_j lies in span(V_{j+2}) to the bound of ``recurrences.arnoldi_tol``
    (whole rows and their last 4 096 elements); the device solution is the float64 least-squares solution over V_k, and over
    V_5 for the truncated form; the Givens residuals are the true float64 residuals; base + scale * V y is one rounding of
    its float64 value; ``residual_norms`` stores g = fx - x, -g exactly and states their fp32 norms."""
    nat = pkg("_native")
    if reorth == "always":
        knobs(PSIGNN_GMRES_REORTH="always")
    (gm, k, a64, bd), ran = _profiled(lambda: _gmres(M, dev, 20, 0.0))
    where = f"gmres M={M} {reorth}"
    chain = 16 if M >= VEC16_FROM else 4
    assert k == 20, (where, k)
    assert ran["k_gm_finish"][0] == k and ran["k_gm_dots"][0] == ran["k_gm_axpy"][0] == 2 * k, (where, ran)
    assert ran["k_gm_decide"][0] == ran["k_gm_scale"][0] == k, (where, ran)
    if reorth == "always":
        assert gm.reorth_count() == k
    V = gm.V[:k + 1, :M].cpu()
    b = bd.cpu()
    hist = gm.history()
    rc.check_gmres_history(b, hist, k, where)
    AV = rc.check_gmres_basis(a64, V, k, where, chain=chain)
    z = torch.empty_like(bd)
    kk, beta, resid = gm.solution(None, 1.0, z, info=True)
    assert kk == k and resid == hist[k], (kk, k, resid, hist[k])
    rc.check_gmres_solution(a64, b, V, k, z.cpu(), hist, where, AV, chain=chain)
    z5 = torch.empty_like(bd)
    gm.solution(None, 1.0, z5, k=5)
    rc.check_gmres_solution(a64, b, V, 5, z5.cpu(), hist, f"{where} k=5", AV, chain=chain)
    gen = torch.Generator().manual_seed(6)
    base = torch.randn(M, generator=gen)
    out = torch.empty_like(bd)
    gm.solution(base.to(dev), 0.5, out)
    want = base.double() + 0.5 * z.cpu().double()
    err = (out.cpu().double() - want).abs()
    assert bool((err <= rc.EPS32 * want.abs()).all()), (where, "base + scale * V y", int(err.argmax()), float(err.max()))
    x = torch.randn(M, generator=gen).to(dev)
    fx = torch.randn(M, generator=gen).to(dev)
    g, ng = torch.empty_like(x), torch.empty_like(x)
    n_g, n_f = gm.residual_norms(x, fx, g, ng)
    assert torch.equal(g, fx - x) and torch.equal(ng, -(fx - x)), where
    rc._norm_close(n_g, (fx - x).cpu(), f"{where} |fx - x|")
    rc._norm_close(n_f, fx.cpu(), f"{where} |fx|")
    gm.close()
    if reorth == "always":
        knobs(PSIGNN_GMRES_REORTH=None)


def test_gmres_krylov_space_runs_out(dev):
    """M = 10 unknowns, m_max = 20, eta = 1e-6: the Krylov space is the whole space after 10 steps; the solve stops by step 11
    with the float64 solution to fp32 accuracy, and nothing in the solution or the residual history is NaN or inf."""
    gm, k, a64, bd = _gmres(10, dev, 20, 1e-6)
    assert k <= 11, k
    z = torch.empty_like(bd)
    gm.solution(None, 1.0, z)
    hist = gm.history()
    assert bool(torch.isfinite(z).all()) and all(np.isfinite(hist)), (z, hist)
    A = torch.stack([a64(e) for e in torch.eye(10, dtype=torch.float64)], 1)
    want = torch.linalg.solve(A, bd.cpu().double())
    assert rel_l2(z, want) < 1e-5, rel_l2(z, want)
    rc.check_gmres_history(bd.cpu(), hist, k, "run-out")
    gm.close()


@pytest.mark.parametrize("M", [4090, 1000010])
def test_gmres_zero_rhs(M, dev):
    """b = 0: the solve stops before its first step, and solution(base, scale) is base itself, finite."""
    gm, k, _, bd = _gmres(M, dev, 8, 1e-6, zero_rhs=True)
    assert k == 1, k                                    # the first step already reports done
    gen = torch.Generator().manual_seed(7)
    base = torch.randn(M, generator=gen).to(dev)
    out = torch.empty_like(base)
    kk, beta, resid = gm.solution(base, 0.5, out, info=True)
    assert kk == 0 and beta == 0.0 and resid == 0.0, (kk, beta, resid)
    assert torch.equal(out, base) and bool(torch.isfinite(out).all())
    gm.close()
