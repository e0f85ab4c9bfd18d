"""The float64 step checkers of tests/recurrences.py, without a GPU: each accepts a trajectory made on the CPU (the oracle's
Anderson / Picard, a float32 Arnoldi in torch) and rejects corrupted copies of it -- a checker that always passes would look
the same as a kernel that is right."""
import pytest
import torch

import recurrences as rc
from oracle import psignn_oracle as orc


def _map(N, seed=0, nonlinear=False, rho=0.6):
    """f(x) = c * x + s * roll(x, 7) + b (|c| + |s| <= rho: a contraction, coupled across elements), or c * tanh(x) + b."""
    gen = torch.Generator().manual_seed(seed)
    c = 0.05 + (rho - 0.25) * torch.rand(N, 10, generator=gen)
    s = 0.4 * (torch.rand(N, 10, generator=gen) - 0.5)
    b = torch.randn(N, 10, generator=gen)
    x0 = torch.randn(N, 10, generator=gen)
    if nonlinear:
        return (lambda x: c * torch.tanh(x) + b), x0
    return (lambda x: c * x + s * torch.roll(x, 7) + b), x0


def _fails(match, fn, *a, **kw):
    with pytest.raises(AssertionError, match=match):
        fn(*a, **kw)


@pytest.mark.parametrize("m", [2, 5, 8])
@pytest.mark.parametrize("beta", [1.0, 0.6])
def test_anderson_checker(m, beta):
    f, x0 = _map(60, seed=m, rho=0.95)       # slow enough that the history is still far from converged when the ring wraps
    T = 30
    rec = rc.Recorder(f)
    out = orc.anderson(rec, x0, m=m, lam=1e-4, threshold=T, eps=0.0, beta=beta)
    P, R = rec.P, rec.R
    assert rc.check_anderson(P, R, out, m, 1e-4, beta, T, 0.0) == T - 2
    # F slots 0 and 1 swapped against the X slots in one mixing step (after the ring has wrapped)
    k = m + 2
    n, js = rc.anderson_slots(k, m)
    Xs, Fs = torch.stack([P[j] for j in js]), torch.stack([R[j] for j in js])
    Fs = Fs[[1, 0] + list(range(2, n))]
    bad = list(P)
    bad[k] = rc.anderson_mix(Xs, Fs, 1e-4, beta, torch.float32)
    _fails(f"step k={k}'", rc.check_anderson, bad, R, out, m, 1e-4, beta, T, 0.0)
    # the last two elements of one trial point off by 1e-3 relative
    bad = list(P)
    bad[k] = P[k].clone()
    bad[k][-2:] *= 1.001
    _fails(f"step k={k}'", rc.check_anderson, bad, R, out, m, 1e-4, beta, T, 0.0)
    # wrong beta; lam dropped (it matters once |G|^2 is down to lam: the later steps)
    _fails("step k=2'", rc.check_anderson, P, R, out, m, 1e-4, 0.8 if beta == 1.0 else 1.0, T, 0.0)
    _fails("step k=", rc.check_anderson, P, R, out, m, 0.0, beta, T, 0.0)
    # a wrong ring order: the checker's slot map off by one
    _fails("step k=", rc.check_anderson, P, R, out, m + 1, 1e-4, beta, T, 0.0)


def test_anderson_checker_early_stop_and_abs_mode():
    f, x0 = _map(40, seed=3, nonlinear=True)
    T = 40
    for mode, eps in (("rel", 1e-5), ("abs", 1e-4)):
        rec = rc.Recorder(f)
        out = orc.anderson(rec, x0, m=3, lam=1e-4, threshold=T, eps=eps, stop_mode=mode)
        n = rc.check_anderson(rec.P, rec.R, out, 3, 1e-4, 1.0, T, eps, stop_mode=mode)
        assert n < T - 2, (mode, n)
        bad = dict(out, nstep=out["nstep"] - 1)
        _fails("nstep", rc.check_anderson, rec.P, rec.R, bad, 3, 1e-4, 1.0, T, eps, stop_mode=mode)
        bad = dict(out, rel_trace=out["rel_trace"][:n] + [0.0] * (T - 2 - n), abs_trace=out["abs_trace"][:n] + [0.0] * (T - 2 - n))
        _fails("padding", rc.check_anderson, rec.P, rec.R, bad, 3, 1e-4, 1.0, T, eps, stop_mode=mode)


@pytest.mark.parametrize("nonlinear", [False, True])
def test_picard_checker(nonlinear):
    f, x0 = _map(50, seed=4, nonlinear=nonlinear)
    rec = rc.Recorder(f)
    out = orc.forward_iteration(rec, x0, eps=1e-5, threshold=60)
    n = rc.check_picard(rec.P, rec.R, out, 60, 1e-5)
    assert 5 < n < 61
    bad = list(rec.P)
    bad[4] = bad[4].clone()
    bad[4][-2:] *= 1.001
    _fails("z_{i\\+1} != f\\(z_i\\)", rc.check_picard, bad, rec.R, out, 60, 1e-5)
    _fails("stop index", rc.check_picard, rec.P, rec.R, out, 60, 1e-3)
    bad = dict(out, abs_trace=[a * (1 + 1e-4) for a in out["abs_trace"]])
    _fails("abs\\[0\\]", rc.check_picard, rec.P, rec.R, bad, 60, 1e-5)
    bad = dict(out, result=torch.as_tensor(rec.P[n - 1]))
    _fails("last iterate", rc.check_picard, rec.P, rec.R, bad, 60, 1e-5)


def _gmres_cpu(M, k, seed=6):
    """float32 Arnoldi (modified Gram-Schmidt, twice; inner products rounded to float32 from float64, like the device's
    partial sums) on A = J - I, J v = c * v + s * roll(v, 7): basis rows, Givens-equivalent residual history, solution."""
    gen = torch.Generator().manual_seed(seed)
    c = 0.05 + 0.35 * torch.rand(M, generator=gen)
    s = 0.4 * (torch.rand(M, generator=gen) - 0.5)
    b = torch.randn(M, generator=gen)
    a32 = lambda v: c * v + s * torch.roll(v, 7) - v
    c64, s64 = c.double(), s.double()
    a64 = lambda v: c64 * v + s64 * torch.roll(v, 7) - v
    V = torch.zeros(k + 1, M)
    H = torch.zeros(k + 1, k, dtype=torch.float64)
    beta = float(b.double().norm())
    V[0] = b * (1.0 / torch.tensor(beta, dtype=torch.float32))
    for j in range(k):
        w = a32(V[j])
        for _ in range(2):
            for i in range(j + 1):
                h = torch.tensor(float(V[i].double() @ w.double()), dtype=torch.float32)
                w = w - h * V[i]
                H[i, j] += float(h)
        hn = float(w.double().norm())
        H[j + 1, j] = hn
        V[j + 1] = w * (1.0 / torch.tensor(hn, dtype=torch.float32))
    e1 = torch.zeros(k + 1, dtype=torch.float64)
    e1[0] = beta
    hist = [beta]
    for i in range(1, k + 1):
        y = torch.linalg.lstsq(H[:i + 1, :i], e1[:i + 1, None]).solution[:, 0]
        hist.append(float((e1[:i + 1] - H[:i + 1, :i] @ y).norm()))
    z = (y.float() @ V[:k])
    return a64, b, V, hist, z


def test_gmres_checker():
    """M = 100: a 1e-3 change of two elements of a unit row moves its norm by ~ 4e-5, above the bound of ``arnoldi_tol``
    (8.6e-6 at k = 12, a worst case: this trajectory itself stays at 1.5e-7)."""
    M, k = 100, 12
    a64, b, V, hist, z = _gmres_cpu(M, k)
    rc.check_gmres_history(b, hist, k, "cpu")
    AV = rc.check_gmres_basis(a64, V, k, "cpu")
    rc.check_gmres_solution(a64, b, V, k, z, hist, "cpu", AV)
    # the last two elements of one basis row off by 1e-3 relative; one basis row with its last 6 elements zeroed
    for what in ("perturbed", "zeroed"):
        bad = V.clone()
        if what == "perturbed":
            bad[5, -2:] *= 1.001
        else:
            bad[5, -6:] = 0.0
        _fails("V\\^T V - I|outside span", rc.check_gmres_basis, a64, bad, k, "cpu")
    # the solution's tail off; a Givens residual that is not the true residual
    bad = z.clone()
    bad[-2:] *= 1.001
    _fails("solution vs float64|Givens residual", rc.check_gmres_solution, a64, b, V, k, bad, hist, "cpu", AV)
    bad = list(hist)
    bad[k] = hist[k] * 1.5 + 1e-3 * hist[0]
    _fails("Givens residual", rc.check_gmres_solution, a64, b, V, k, z, bad, "cpu", AV)
    bad = list(hist)
    bad[3] = bad[2] * 1.01
    _fails("not monotone", rc.check_gmres_history, b, bad, k, "cpu")


def test_broyden_iteration_checker_sees_the_tail():
    """The Broyden recurrence check on a CPU float32 iteration of M = 200 000 elements: accepted; the last two elements of
    the next update off by 1e-3 relative: rejected -- by the tail slice (the whole-vector norm dilutes them by ~ 7 x)."""
    gen = torch.Generator().manual_seed(9)
    M, k = 200000, 3
    U32 = torch.randn(k, M, generator=gen) / M ** 0.5
    V32 = torch.randn(k, M, generator=gen) / M ** 0.5
    dx, dg, g = (torch.randn(M, generator=gen) for _ in range(3))
    U, V = U32.double(), V32.double()
    vT = (-dx + (U @ dx.double()) @ V).float()                  # the device's quantities: float64 results rounded to float32
    u = ((dx + dg).double() - (V @ dg.double()) @ U) / float(vT.double() @ dg.double())
    upd = (g.double() - (V @ g.double()) @ U - u * float(vT.double() @ g.double())).float()
    u = u.float()
    rc._check_iteration(k, U32, V32, U, V, dx, dg, g, vT, u, upd, "cpu")
    bad = upd.clone()
    bad[-2:] *= 1.001
    _fails("cpu tail", rc._check_iteration, k, U32, V32, U, V, dx, dg, g, vT, u, bad, "cpu")
