"""The stop rules of ``broyden`` (reference: utilities/solver.py:163-192), restated once, and maps with a scripted residual.

``replay`` walks the traces a solve returned and says where the reference's rules first fire, why, which step is the lowest and
how the traces are padded.  The device states the same rules twice (``check_block`` in csrc/solver.hip, ``k_b64_test`` in
csrc/solver_f64.hip); both keep their traces as doubles and decide in doubles, so a solve must equal the replay of its own traces
exactly: integers and copied doubles, no tolerance.  tests/test_host_broyden_stop.py pins ``replay`` to ``oracle.broyden`` first.

``Script`` is a map whose residual is known in advance whatever the solver does to the iterate.  With R_n the rotation of element
pairs (a, b) -> +-(-b, a), |R_n(x)| = |x| and R_n(x) is orthogonal to x, so

    rel script:  f_n(x) = x + rho_n R_n(x)                 rel_n = |g| / (|f(x)| + 1e-9) = rho_n / sqrt(1 + rho_n^2)
    abs script:  f_n(x) = x + (a_n |x0| / |x|) R_n(x)      abs_n = |g| = a_n |x0|

Call 0 is g(x0) and no trace entry; trace entry i (step i) is call i.  The sign of each pair's rotation is drawn anew for every
call.  With one fixed rotation g is the linear map rho R x with two eigenvalues, and Broyden learns it: measured on the CPU oracle,
in float64 |x| falls to 1e-8 within 20 steps (where the 1e-9 of the denominator takes rel below the script), and in abs mode |x|
grows to 1e6 |x0| (where fp32 cancellation in f(x) - x puts the trace 70 % off).  With the signs redrawn the secant pairs teach
nothing, and |x| stayed within 1 ... 1.6e3 |x0| on every case, shape, mode and dtype.  ``CASES`` scripts every outcome of the rules and the
off-by-one edges around them, every value at least 1 % (the ratios 1.29 / 1.31: 0.8 %) from the boundary next to it, so that
neither the rounding of the fp32 map nor the order of a multiplication decides a case.  Probed on the CPU oracle in fp32: the trace
follows the script to 1e-5 relative while rho >= 1e-3 and to 6e-4 at rho ~ 1e-5 (cancellation in f(x) - x)."""
import math
from collections import namedtuple

import numpy as np
import torch

REASONS = {0: "threshold", 1: "tolerance", 2: "stagnation", 3: "protective break"}


def replay(rel_trace, abs_trace, n_iter, eps, threshold, seq_len, stop_mode="rel"):
    """The reference's loop (solver.py:160-197) over the first ``n_iter`` entries of the returned traces, in Python doubles.

    Returns ``n_iter`` (the step at which a rule first fires), ``stop_reason`` (0 threshold, 1 tolerance, 2 stagnation, 3 protective
    break), ``prot_break``, ``lowest``, ``nstep`` (the step of the lowest value in ``stop_mode``) and both traces padded to
    ``threshold + 1`` entries with the two lowest values.  When the traces end before any rule fires (the solve stopped too early)
    ``stop_reason`` is None and ``n_iter`` is the number of entries walked."""
    given = {"rel": [float(v) for v in rel_trace[:n_iter]], "abs": [float(v) for v in abs_trace[:n_iter]]}
    alt = "rel" if stop_mode == "abs" else "abs"
    protect_thres = (1e6 if stop_mode == "abs" else 1e3) * seq_len
    trace = {"abs": [], "rel": []}
    lowest = {"abs": 1e8, "rel": 1e8}
    lowest_step = {"abs": 0, "rel": 0}
    prot_break = False
    reason = None
    nstep = 0
    while nstep < threshold:
        if nstep >= len(given[stop_mode]):
            break
        nstep += 1
        diff = {"abs": given["abs"][nstep - 1], "rel": given["rel"][nstep - 1]}
        trace["abs"].append(diff["abs"])
        trace["rel"].append(diff["rel"])
        for mode in ("rel", "abs"):
            if diff[mode] < lowest[mode]:
                lowest[mode] = diff[mode]
                lowest_step[mode] = nstep
        obj = diff[stop_mode]
        if obj < eps:
            reason = 1
            break
        if obj < 3 * eps and nstep > 30 and np.max(trace[stop_mode][-30:]) / np.min(trace[stop_mode][-30:]) < 1.3:
            reason = 2
            break
        if obj > trace[stop_mode][0] * protect_thres:
            prot_break = True
            reason = 3
            break
    else:
        reason = 0
    for _ in range(threshold + 1 - len(trace[stop_mode])):
        trace[stop_mode].append(lowest[stop_mode])
        trace[alt].append(lowest[alt])
    return {"n_iter": nstep, "stop_reason": reason, "prot_break": prot_break, "lowest": lowest[stop_mode],
            "nstep": lowest_step[stop_mode], "rel_trace": trace["rel"], "abs_trace": trace["abs"]}


def _same_doubles(a, b):
    """Equal as lists of doubles, bit for bit (NaN equals NaN: a copied double is the same double)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.int64), b.view(np.int64)))


def assert_replay(out, eps, threshold, seq_len, stop_mode, n_iter=None, what=""):
    """Everything a solve reports against ``replay`` of its own traces; returns the replay.  ``out``: the dictionary of a device
    solve, or the oracle's with ``n_iter`` given (the oracle reports neither the step count nor the reason)."""
    n = out["n_iter"] if n_iter is None else n_iter
    rp = replay(out["rel_trace"], out["abs_trace"], n, eps, threshold, seq_len, stop_mode)
    tag = (what, stop_mode, eps, threshold)
    assert rp["stop_reason"] is not None, ("stopped at a step where no rule fires", n, *tag)
    assert rp["n_iter"] == n, ("the rules fire at another step", rp["n_iter"], n, rp["stop_reason"], *tag)
    if "stop_reason" in out:
        assert out["stop_reason"] == rp["stop_reason"], (out["stop_reason"], rp["stop_reason"], *tag)
    assert bool(out["prot_break"]) == rp["prot_break"] == (rp["stop_reason"] == 3), (out["prot_break"], rp["stop_reason"], *tag)
    assert out["nstep"] == rp["nstep"], (out["nstep"], rp["nstep"], *tag)
    assert _same_doubles([out["lowest"]], [rp["lowest"]]), (out["lowest"], rp["lowest"], *tag)
    assert len(out["rel_trace"]) == len(out["abs_trace"]) == threshold + 1, (len(out["rel_trace"]), *tag)
    assert _same_doubles(out["rel_trace"], rp["rel_trace"]), ("rel_trace", *tag)
    assert _same_doubles(out["abs_trace"], rp["abs_trace"]), ("abs_trace", *tag)
    return rp


# ------------------------------------------------------------------------------------------------------- scripted maps
_SIGNS = {}


def _signs(pairs, n, device):
    """+-1 per element pair for call n (int8; drawn on the CPU from a generator seeded with n, so every device sees the same)."""
    key = (pairs, n, str(device))
    if key not in _SIGNS:
        gen = torch.Generator().manual_seed(1000 + n)
        _SIGNS[key] = (torch.randint(0, 2, (pairs,), generator=gen, dtype=torch.int8) * 2 - 1).to(device)
    return _SIGNS[key]


def rotate_pairs(x, n=None):
    """R_n: (a, b) -> s (-b, a) on consecutive element pairs of the flattened tensor, s = +-1 per pair drawn anew for every call n
    (``n=None``: s = 1).  An odd last element maps to 0: a start vector whose last element is 0 keeps it 0 in every vector the
    iteration forms, so |R_n(x)| = |x| still holds there."""
    flat = x.reshape(-1)
    m = flat.numel() // 2 * 2
    y = flat[:m].reshape(-1, 2)
    if n is not None:
        y = y * _signs(m // 2, n, x.device).to(x.dtype)[:, None]
    r = torch.zeros_like(flat)
    r[:m] = torch.stack([-y[:, 1], y[:, 0]], 1).reshape(-1)
    return r.reshape(x.shape)


def start_vector(shape, device=None, dtype=None, seed=0):
    """randn(shape), the last element 0 when the element count is odd (``rotate_pairs``)."""
    gen = torch.Generator().manual_seed(seed)
    x0 = torch.randn(shape, generator=gen, dtype=dtype)
    if x0.numel() % 2:
        x0.reshape(-1)[-1] = 0.0
    return x0.to(device) if device is not None else x0


class Script:
    """The scripted map: counts its calls and keeps a clone of every x it is handed (``xs[i]`` is the x of call i).  ``values[n]``
    is the residual of call n in ``stop_mode`` -- rel_n itself, or abs_n in units of |x0| -- the last value repeating."""

    def __init__(self, values, stop_mode, x0):
        self.values, self.mode = list(values), stop_mode
        self.x0_norm = float(x0.double().norm())
        self.calls, self.xs = 0, []

    def __call__(self, x):
        n = self.calls
        v = self.values[min(n, len(self.values) - 1)]
        self.calls += 1
        self.xs.append(x.clone())
        if self.mode == "rel":
            return x + (v / math.sqrt(1.0 - v * v)) * rotate_pairs(x, n)
        return x + (v * self.x0_norm / float(x.double().norm())) * rotate_pairs(x, n)

    def eps(self, eps):
        """The case's tolerance in this script's units (abs: scaled by |x0| like the values)."""
        return eps if self.mode == "rel" else eps * self.x0_norm


# ---------------------------------------------------------------------------------------------------------------- cases
def _w(i, a):
    """1 ... 1 + a, every fifth entry at either end: the max / min of any 5 consecutive entries is 1 + a."""
    return 1 + a * ((i * 7) % 5) / 4


def _plateau(level, a, head=()):
    return [0.5] + list(head) + [level * _w(i, a) for i in range(50)]


def _break(d, first, factor):
    """``first`` at step 1, the lowest (half of it) at step 3, then 0.5, 0.9 and 1.2 times the limit ``first * factor * d``."""
    lim = first * factor * d
    return [0.5, first, 2 * first, 0.5 * first, 0.5 * lim, 0.9 * lim, 1.2 * lim]


# name; values(d, stop_mode): the script from call 0 on; eps (rel units); threshold; the stop that must come out: reason, step, and
# the step of the lowest where the script fixes it (None: several entries share the lowest scripted value); d: the widths it is for
Case = namedtuple("Case", "name values eps threshold reason step nstep widths")
EPS = 1e-3
CASES = [
    Case("tolerance_at_5", lambda d, m: [0.5, 0.1, 0.05, 1.01 * EPS, 1.01 * EPS, 0.99 * EPS, 0.3], EPS, 45, 1, 5, 5, None),
    Case("stagnation_at_31", lambda d, m: _plateau(2 * EPS, 0.1), EPS, 45, 2, 31, None, None),
    Case("ratio_1.29", lambda d, m: _plateau(2 * EPS, 0.29), EPS, 45, 2, 31, None, None),
    Case("ratio_1.31", lambda d, m: _plateau(2 * EPS, 0.31), EPS, 45, 0, 45, None, None),
    Case("below_3eps", lambda d, m: _plateau(2.75 * EPS, 0.05), EPS, 45, 2, 31, None, None),
    Case("above_3eps", lambda d, m: _plateau(3.1 * EPS, 0.05), EPS, 45, 0, 45, None, None),
    Case("window_is_30", lambda d, m: [0.5] + [2 * EPS * (1.5 if i < 10 else _w(i, 0.1)) for i in range(50)], EPS, 45, 2, 40, None, None),
    Case("lowest_not_last", lambda d, m: _plateau(2 * EPS, 0.1, head=[5 * EPS, 4 * EPS, 1.5 * EPS, 4 * EPS, 5 * EPS]), EPS, 45, 2, 35, 3, None),
    # rel: 1e-5, 2e-5, 5e-6, then 0.5 / 0.9 / 1.2 x the limit 1e-5 * 1e3 * d (d = 10: 5e-2, 9e-2, 0.12).  abs: 1e-4 |x0| first, the
    # limit 1e-4 * 1e6 * d |x0| (d = 10: 1.2e3 |x0| at step 6)
    Case("protective_break", lambda d, m: _break(d, 1e-5, 1e3) if m == "rel" else _break(d, 1e-4, 1e6), 1e-9, 45, 3, 6, 3, None),
    # seq_len reaches the kernel: the limit is 0.07 at d = 7 (9e-2 at step 5 is past it) and 0.1 at d = 10 (nothing is)
    Case("seq_len_7_breaks", lambda d, m: [0.5, 1e-5, 2e-5, 5e-6, 5e-2, 9e-2, 0.085], 1e-9, 45, 3, 5, 3, (7,)),
    Case("seq_len_10_does_not", lambda d, m: [0.5, 1e-5, 2e-5, 5e-6, 5e-2, 9e-2, 0.085], 1e-9, 45, 0, 45, 3, (10,)),
]
CASE = {c.name: c for c in CASES}
LONG_CASES = ("stagnation_at_31", "lowest_not_last", "protective_break")


def cases_for(d, stop_mode):
    """The cases that run at width ``d`` in ``stop_mode`` (the two seq_len cases are stated for the rel limit)."""
    return [c for c in CASES if c.widths is None or (d in c.widths and stop_mode == "rel")]


def run_case(case, solve, x0, stop_mode):
    """``solve(script, x0, threshold, eps)`` -> the solver's dictionary, on a fresh script of ``case``; asserts what the case names
    and what ``replay`` says; returns (out, script, replay)."""
    d = x0.shape[1]
    sc = Script(case.values(d, stop_mode), stop_mode, x0)
    eps = sc.eps(case.eps)
    out = solve(sc, x0, case.threshold, eps)
    n_iter = sc.calls - 1
    what = f"{case.name} {tuple(x0.shape)}"
    assert out.get("n_iter", n_iter) == n_iter, (what, out.get("n_iter"), n_iter)
    rp = assert_replay(out, eps, case.threshold, d, stop_mode, n_iter=n_iter, what=what)
    assert (rp["stop_reason"], n_iter) == (case.reason, case.step), (what, stop_mode, rp["stop_reason"], n_iter)
    if case.nstep is not None:
        assert out["nstep"] == case.nstep, (what, stop_mode, out["nstep"])
    assert torch.equal(out["result"].reshape(x0.shape), sc.xs[out["nstep"]].reshape(x0.shape)), (what, stop_mode, "result is not iterate nstep")
    return out, sc, rp
