"""Float64 step checkers of the device solvers (Broyden update, Anderson, Picard, GMRES).

A float32 trajectory of any of these solvers cannot be compared with a float64 one over many steps: the iterations are
chaotic in float32 (every Broyden update divides by a difference of nearly equal numbers; Anderson's bordered solve grows
ill-conditioned as the residual history converges).  What can be checked, at every step, is the step by itself: recompute it
in float64 on the CPU from the device's OWN previous state (recorded by wrapping f) and compare.

The tolerance is not fitted.  A device quantity may be at most 16 x as far from the float64 value as a plain float32 torch
evaluation of the same formula is (``_scale``), plus a floor of a few ulp of its norm.  GMRES, whose basis is compared with
exact properties (orthonormality, the Arnoldi relation), uses a bound derived from the fp32 unit roundoff (``arnoldi_tol``).

Every check is made twice: over the whole vector and over its last ``TAIL`` elements (the whole vector when it is shorter),
with the tolerance computed on that slice -- an error confined to the ragged last block of a long vector is diluted by
sqrt(M / tail) in a whole-vector norm and would hide below the tolerance there."""
import numpy as np
import torch

EPS32 = float(np.finfo(np.float32).eps)
U32 = EPS32 / 2          # fp32 unit roundoff
TAIL = 4096


def tail(M):
    return slice(max(0, M - TAIL), M)


def _scale(ref64, plain32):
    """Rounding scale of a formula: distance of its plain float32 evaluation from the float64 one (plus a floor of 4 ulp)."""
    return float((plain32.double() - ref64).norm()) + 4 * EPS32 * float(ref64.norm())


def _near(got, ref64, plain32, what, sl=None):
    """|got - ref64| <= 16 * _scale over the whole vector and over the tail slice (``sl``: default ``tail``)."""
    sl = tail(ref64.numel()) if sl is None else sl
    for part, name in ((slice(None), "all"), (sl, "tail")):
        e = float((got[part].double() - ref64[part]).norm())
        s = _scale(ref64[part], plain32[part])
        assert e <= 16 * s, (what, name, e, s)


# ---------------------------------------------------------------------------------------------------------- Broyden
def _check_iteration_on(U32m, V32m, U, V, dx, dg, g, Vk, Uk, upd_next, where, c_vT, c_D1, c_D2, glob=None):
    """The three recurrences on one slice of the vectors.  c_*: the pair coefficients (U dx, V dg, V g) in float64 and
    float32, computed over the WHOLE vectors; ``glob``: for a slice, (proj, beta, tol_dir, tol2 / |U_k|) of the whole-vector
    check -- the coefficients fitted there, whose own uncertainty enters the slice's tolerance."""
    dxd, dgd, gd = dx.double(), dg.double(), g.double()
    # vT = -dx + (U dx) V
    vT = -dxd + c_vT[0] @ V
    vT32 = -dx + c_vT[1] @ V32m
    e = float((Vk.double() - vT).norm())
    assert e <= 16 * _scale(vT, vT32), (where, "vT", e, _scale(vT, vT32))
    # u = D1 / s,  D1 = dx + dg - (V dg) U,  s = vT . dg  (the device's own vT: the stages are checked one by one)
    D1 = dxd + dgd - c_D1[0] @ U
    D1_32 = dx + dg - c_D1[1] @ U32m
    Ukd = Uk.double()
    tol_dir = 16 * _scale(D1, D1_32) / float(D1.norm())
    if glob is None:
        proj = float(D1 @ Ukd) / float(D1 @ D1)                   # U_k = proj * D1 + remainder, proj = 1 / s
        rem = float((Ukd - proj * D1).norm())
        assert rem <= tol_dir * float(Ukd.norm()), (where, "U_k direction", rem / float(Ukd.norm()), tol_dir)
        s64 = float(Vk.double() @ dgd)
        s_abs = float((Vk.double() * dgd).abs().sum())
        assert abs(1.0 / proj - s64) <= 16 * EPS32 * s_abs + 4 * tol_dir * abs(s64), (where, "s = vT.dg", 1.0 / proj, s64, s_abs)
    else:
        proj, _, tol_dir_all, _ = glob
        rem = float((Ukd - proj * D1).norm())
        assert rem <= (tol_dir + tol_dir_all) * float(Ukd.norm()), (where, "U_k direction", rem / float(Ukd.norm()), tol_dir)
    # update = D2 - u beta,  D2 = g - (V g) U,  beta = vT . g
    D2 = gd - c_D2[0] @ U
    D2_32 = g - c_D2[1] @ U32m
    r = D2 - upd_next.double()
    tol2 = 16 * _scale(D2, D2_32)
    if glob is None:
        beta = float(r @ Ukd) / float(Ukd @ Ukd)
        rem2 = float((r - beta * Ukd).norm())
        tol2 += 8 * EPS32 * (float(D2.norm()) + abs(beta) * float(Ukd.norm()))
        assert rem2 <= tol2, (where, "update", rem2, tol2)
        b64 = float(Vk.double() @ gd)
        b_abs = float((Vk.double() * gd).abs().sum())
        assert abs(beta - b64) <= 16 * EPS32 * b_abs + 4 * (tol2 / float(Ukd.norm())), (where, "beta = vT.g", beta, b64, b_abs)
        return proj, beta, tol_dir, tol2 / float(Ukd.norm())
    _, beta, _, dbeta = glob
    rem2 = float((r - beta * Ukd).norm())
    tol2 += 8 * EPS32 * (float(D2.norm()) + abs(beta) * float(Ukd.norm())) + dbeta * float(Ukd.norm())
    assert rem2 <= tol2, (where, "update", rem2, tol2)


def _check_iteration(k, U32, V32, U, V, dx, dg, g, Vk, Uk, upd_next, where):
    """Iteration with k stored pairs (all CPU tensors; U32, V32: (k, M) float32, U, V the same in float64): the device's V_k, U_k
    and next update against the float64 recurrences on the device's own previous state -- over the whole vectors, then over
    the tail slice with the same (whole-vector) pair coefficients."""
    dxd, dgd, gd = dx.double(), dg.double(), g.double()
    c_vT, c_D1, c_D2 = (U @ dxd, U32 @ dx), (V @ dgd, V32 @ dg), (V @ gd, V32 @ g)
    glob = _check_iteration_on(U32, V32, U, V, dx, dg, g, Vk, Uk, upd_next, where, c_vT, c_D1, c_D2)
    sl = tail(dx.numel())
    _check_iteration_on(U32[:, sl], V32[:, sl], U[:, sl], V[:, sl], dx[sl], dg[sl], g[sl], Vk[sl], Uk[sl], upd_next[sl],
                        f"{where} tail", c_vT, c_D1, c_D2, glob)


# ------------------------------------------------------------------------------------- host-driven Broyden run, recorded
K = 48          # iterations per recorded solve unless told otherwise: the window regime starts at k = 25 with the default limits


class _Recorder:
    """Wraps f for ``DeviceBroyden.solve_callable``: keeps every evaluation point and, from the second call on, the solver's
    update vector at the time of the call (= dx of that iteration: x_new = x + update has just been formed)."""

    def __init__(self, f, back=lambda t: t):
        self.f, self.back, self.solver = f, back, None
        self.X, self.DX = [], []

    def __call__(self, x):
        if self.X:
            self.DX.append(self.solver.pair(0, self.back(x), "update"))
        self.X.append(self.back(x).clone())
        return self.f(x)


def _run_recorded(eng, f, x0, n_elems=None, plan=None, shard_elems=0, back=lambda t: t, K=K):
    rec = _Recorder(f, back)
    if plan is not None:
        sv = eng.DeviceBroyden(plan=plan, threshold=K, keep_trace=True, shard_elems=shard_elems)
    else:
        sv = eng.DeviceBroyden(threshold=K, keep_trace=True, n_elems=n_elems, seq_len=x0.shape[1], device=x0.device)
    rec.solver = sv
    out = sv.solve_callable(rec, x0, 0.0)
    assert out["n_iter"] == K and out["stop_reason"] == 0, (out["n_iter"], out["stop_reason"])
    rec.DX.append(sv.pair(0, back(x0), "update"))        # the update formed by the last iteration
    return rec, sv, out


def _check_run(rec, sv, its, label, K=K):
    """rec.X[i] = iterate i (i = 0 .. K), rec.DX[i] = update that led from iterate i to i + 1 (and DX[K] the one after)."""
    X, DX = rec.X, rec.DX
    assert len(X) == K + 1 and len(DX) == K + 1
    for i in (1, K // 2, K):                                      # the recorded points are the solver's iterates
        assert torch.equal(sv.iterate(i, X[0]), X[i])
    kmax = max(its)
    Ucpu = torch.stack([sv.pair(j, X[0], "U").reshape(-1).cpu() for j in range(kmax + 1)])
    Vcpu = torch.stack([sv.pair(j, X[0], "V").reshape(-1).cpu() for j in range(kmax + 1)])
    U64, V64 = Ucpu.double(), Vcpu.double()
    G = {}

    def gof(i):                                                   # g_i = f(x_i) - x_i in float32, as k_resid forms it
        if i not in G:
            xi = X[i]
            G[i] = (rec.f(rec.fwd(xi)) if hasattr(rec, "fwd") else rec.f(xi))
            G[i] = (rec.back(G[i]) - xi).reshape(-1).cpu()
        return G[i]

    for it in its:       # iteration `it` (0-based): k = it stored pairs, x_it -> x_{it+1}, stores pair `it`, forms update it+1
        g_new, g_old = gof(it + 1), gof(it)
        _check_iteration(it, Ucpu[:it], Vcpu[:it], U64[:it], V64[:it], DX[it].reshape(-1).cpu(), g_new - g_old, g_new, Vcpu[it], Ucpu[it],
                         DX[it + 1].reshape(-1).cpu(), f"{label} it={it}")


# ---------------------------------------------------------------------------------------------------------- recorder
class Recorder:
    """Wraps f: keeps every evaluation point and every returned value, flattened, on the CPU."""

    def __init__(self, f):
        self.f = f
        self.P, self.R = [], []

    def __call__(self, x):
        y = self.f(x)
        self.P.append(x.detach().reshape(-1).cpu().clone())
        self.R.append(y.detach().to(torch.float32).reshape(-1).cpu().clone())
        return y


def _norm64(vec32):
    """(float64 norm of an fp32 vector, rounding scale of its plain float32 evaluation incl. a 4-ulp floor)."""
    n64 = float(vec32.double().norm())
    return n64, abs(float(vec32.norm()) - n64) + 4 * EPS32 * n64


def _norm_close(got, vec32, what):
    """A norm the device reports (fp32 value) against the float64 norm of the fp32 vector it was formed from."""
    n64, s = _norm64(vec32)
    assert abs(got - n64) <= 16 * s, (what, got, n64, s)
    return n64, s


def _check_traces(P, R, ks, abs_tr, rel_tr, rel_floor, where):
    """abs = |R_k - P_k|, rel = abs / (rel_floor + |R_k|) for the entries i <-> evaluations ks[i] (whole-vector norms by
    definition: the tail is covered by the step checks)."""
    for i, k in enumerate(ks):
        a64, da = _norm_close(abs_tr[i], R[k] - P[k], f"{where} abs[{i}]")
        f64, df = _norm64(R[k])                                   # (the device's |F| is not reported)
        den = rel_floor + f64
        r64 = a64 / den
        tol = 16 * (da / den + r64 * df / den) + 4 * EPS32 * r64
        assert abs(rel_tr[i] - r64) <= tol, (where, "rel", i, rel_tr[i], r64, tol)


# ---------------------------------------------------------------------------------------------------------- Anderson
def anderson_slots(k, m):
    """Loop index k: (n, [j of slot 0 .. n-1]) -- slot s holds the most recent X_j with j = s (mod m), j < k."""
    n = min(k, m)
    return n, [max(j for j in range(k) if j % m == s) for s in range(n)]


def anderson_mix(X, F, lam, beta, dtype):
    """x = beta sum alpha F + (1 - beta) sum alpha X, alpha of [[0, 1^T], [1, G G^T + lam I]] [nu; alpha] = [1; 0]."""
    X, F = X.to(dtype), F.to(dtype)
    n = X.shape[0]
    G = F - X
    H = torch.zeros(n + 1, n + 1, dtype=dtype)
    H[0, 1:] = H[1:, 0] = 1
    H[1:, 1:] = G @ G.T + lam * torch.eye(n, dtype=dtype)
    y = torch.zeros(n + 1, 1, dtype=dtype)
    y[0] = 1
    alpha = torch.linalg.solve(H, y)[1:, 0]
    return beta * (alpha @ F) + (1 - beta) * (alpha @ X)


def check_anderson(P, R, out, m, lam, beta, threshold, eps, stop_mode="rel", where="anderson"):
    """P / R: the recorder's points and values of an ``anderson`` run (P[0] = x0, P[1] = f(x0), P[k] = the trial point of loop
    index k >= 2); ``out``: its result dict.  Every step from the device's own ring slots, the traces, result / nstep, padding."""
    assert torch.equal(P[1], R[0]), (where, "X_1 = f(x0)")
    obj = out["abs_trace"] if stop_mode == "abs" else out["rel_trace"]
    assert len(out["rel_trace"]) == len(out["abs_trace"]) == threshold - 2, (where, len(out["rel_trace"]))
    n_done = next((i + 1 for i, o in enumerate(obj) if o < eps), threshold - 2)
    ks = list(range(2, 2 + n_done))
    assert len(P) >= 2 + n_done, (where, "evaluations", len(P), n_done)
    for k in ks:
        n, js = anderson_slots(k, m)
        Xs, Fs = torch.stack([P[j] for j in js]), torch.stack([R[j] for j in js])
        x64 = anderson_mix(Xs, Fs, lam, beta, torch.float64)
        x32 = anderson_mix(Xs, Fs, lam, beta, torch.float32)
        _near(P[k], x64, x32, f"{where} step k={k}")
    _check_traces(P, R, ks, out["abs_trace"], out["rel_trace"], 1e-5, where)
    low = min(range(n_done), key=lambda i: (obj[i], i))            # first occurrence of the lowest objective
    assert out["nstep"] == low + 2, (where, "nstep", out["nstep"], low + 2)
    assert torch.equal(out["result"].detach().reshape(-1).cpu(), P[low + 2]), (where, "result is not the lowest iterate")
    assert float(out["lowest"]) == obj[low], (where, "lowest", out["lowest"], obj[low])
    if n_done < threshold - 2:    # early stop: padded with the lowest values (solver.py:279-282)
        for tr in (out["rel_trace"], out["abs_trace"]):
            assert all(v == min(tr[:n_done]) for v in tr[n_done:]), (where, "padding", tr[n_done:], min(tr[:n_done]))
    return n_done


# ---------------------------------------------------------------------------------------------------------- Picard
def check_picard(P, R, out, threshold, eps, where="picard"):
    """P / R of a ``forward_iteration`` run: z_{i+1} is bit-identical to f(z_i) as returned, abs = |z_i - f(z_i)|,
    rel = abs / |f(z_i)|; stop at the first rel <= eps (or after threshold loop passes); the result is the last iterate."""
    rel = [float(r) for r in out["rel_trace"]]
    ab = [float(a) for a in out["abs_trace"]]
    n = len(rel)
    stop = next((i + 1 for i, r in enumerate(rel) if not r > eps), threshold + 1)
    assert n == stop, (where, "stop index", n, stop)
    assert out["nstep"] == n - 1, (where, "nstep", out["nstep"], n)
    assert len(P) >= n
    for i in range(n - 1):
        assert torch.equal(P[i + 1], R[i]), (where, "z_{i+1} != f(z_i)", i)
    _check_traces(P, R, list(range(n)), ab, rel, 0.0, where)
    assert torch.equal(out["result"].detach().reshape(-1).cpu(), R[n - 1]), (where, "result is not the last iterate")
    return n


# ---------------------------------------------------------------------------------------------------------- GMRES
def arnoldi_tol(k, chain=16):
    """Bound on |V^T V - I| (entrywise) and on the Arnoldi residual of step k, relative: 4 (chain + 8 + k) u.

    Derivation (u = 2^-24): an inner product accumulates at most ``chain`` fp32 fma per lane (16 floats per lane) and 8 more
    fp32 additions in the wave / block trees before the partials are summed in float64, so its error is at most
    (chain + 8) u |v| |w|; the axpy pass subtracts k + 1 scaled rows, k + 1 more roundings per element of w; the
    normalisation adds 2 u.  The second Gram-Schmidt pass (or the DGKS test that skips it only when |w'| >= |w| / sqrt 2)
    leaves at most twice the single-pass level: factor 2, and another 2 for the operator's own fp32 rounding (3 operations per
    element here) and the ragged summation shapes.  Hence 4 (chain + 8 + k) u: 1.1e-5 for k = 24 at 16 floats per lane."""
    return 4 * (chain + 8 + k) * U32


def check_gmres_basis(apply64, V, k, where, chain=16):
    """V: (>= k + 1, M) float32 rows of the device basis after k Arnoldi steps; apply64: float64 operator A.
    V_k orthonormal (row k: normalised here -- a solve that stopped leaves it unscaled) and A v_j in span(V_{j+2}), j < k,
    over the whole rows and over the tail slice."""
    Vd = V[:k + 1].double()
    nk = float(Vd[k].norm())
    if nk > 0:
        Vd[k] /= nk
    tol = arnoldi_tol(k, chain)
    err = float((Vd @ Vd.T - torch.eye(k + 1, dtype=torch.float64)).abs().max())
    assert err <= tol, (where, "V^T V - I", err, tol)
    sl = tail(V.shape[1])
    AV = []
    for j in range(k):
        w = apply64(V[j].double())
        AV.append(w)
        B = Vd[:j + 2]
        c = torch.linalg.lstsq(B.T, w[:, None]).solution[:, 0]
        r = w - c @ B
        for part, name in ((slice(None), "all"), (sl, "tail")):
            e, s = float(r[part].norm()), float(w[part].norm())
            assert e <= tol * s, (where, f"A v_{j} outside span(V_{j + 2})", name, e / s, tol)
    return AV


def check_gmres_solution(apply64, b, V, kk, z, hist, where, AV=None, chain=16):
    """z: the device's solution from the first kk basis rows.  Against the float64 least-squares minimum of |b - A V_kk y|:
    z = V_kk y* within a relative 1e-4 (whole vector and tail), and the Givens residual hist[kk] equals |b - A z| in float64
    up to the Arnoldi relation's accuracy."""
    bd = b.double()
    Vk = V[:kk].double()
    Y = torch.stack(AV[:kk] if AV is not None else [apply64(v) for v in Vk], 1)
    ys = torch.linalg.lstsq(Y, bd[:, None]).solution[:, 0]
    zs = ys @ Vk
    zd = z.double()
    sl = tail(zd.numel())
    for part, name in ((slice(None), "all"), (sl, "tail")):
        e = float((zd[part] - zs[part]).norm()) / float(zs[part].norm())
        assert e <= 1e-4, (where, "solution vs float64 least squares", name, e)
    true = float((bd - apply64(zd)).norm())
    rmin = float((bd - Y @ ys).norm())
    beta = float(bd.norm())
    tol = 2 * arnoldi_tol(kk, chain) * (beta + float(sum(abs(float(ys[j])) * float(Y[:, j].norm()) for j in range(kk))))
    assert true <= rmin + 1e-4 * beta, (where, "residual above the least-squares minimum", true, rmin)
    assert abs(hist[kk] - true) <= tol, (where, "Givens residual", kk, hist[kk], true, tol)
    return true


def check_gmres_history(b, hist, k, where):
    """hist[0] = |b| (fp32 norm), non-increasing through step k, finite."""
    _norm_close(hist[0], b, f"{where} beta")
    assert all(np.isfinite(hist)), (where, "history not finite", hist)
    assert all(hist[i + 1] <= hist[i] * (1 + 1e-12) for i in range(k)), (where, "history not monotone", hist[:k + 1])
