"""Helpers of tests/test_gpu_handle_reuse.py: comparing two solver dictionaries bit for bit, a handle that is used for a chain of
solves beside fresh handles, and the order in which the scripted cases follow each other on one handle."""
import numpy as np
import torch

import broyden_stop_ref as bsr

_INT_OF = {torch.float32: torch.int32, torch.float64: torch.int64, torch.bfloat16: torch.int16}


def same_tensor(a, b):
    """Equal bit for bit (so NaN equals the same NaN and -0 does not equal +0)."""
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(_INT_OF[a.dtype]), b.contiguous().view(_INT_OF[b.dtype]))


def same_out(a, b, what):
    """Every field of two solver dictionaries: tensors and doubles bit for bit, counters, flags and names with ``==``."""
    assert set(a) == set(b), (what, sorted(a), sorted(b))
    for k in sorted(a):
        va, vb = a[k], b[k]
        if torch.is_tensor(va):
            assert same_tensor(va, vb), (what, k)
        elif isinstance(va, (list, tuple)):
            assert len(va) == len(vb), (what, k, len(va), len(vb))
            if any(isinstance(v, float) for v in va):
                assert bsr._same_doubles(va, vb), (what, k)
            else:
                assert list(va) == list(vb), (what, k)
        elif isinstance(va, float):
            assert bsr._same_doubles([va], [vb]), (what, k, va, vb)
        else:
            assert va == vb, (what, k, va, vb)


def first_entries(out):
    """What a solve saw first: the first entry of every trace it reports (and the right-hand side's norm where it reports one)."""
    return tuple(float(out[k][0]) if len(out[k]) else None for k in ("rel_trace", "abs_trace", "res_trace") if k in out) + \
        ((float(out["b_norm"]),) if "b_norm" in out else ())


def ending(out):
    """How a solve ended, for the REUSE lines."""
    if "stop" in out:            # GMRES
        return f"{out['stop']} after {out['nstep']} products, {out['n_cycles']} cycles"
    if "converged" in out:       # PCG
        return f"{'converged' if out['converged'] else 'not converged'} after {out['n_iter']} iterations"
    reason = bsr.REASONS.get(out["stop_reason"], out["stop_reason"]) if "prot_break" in out else f"stop_reason {out['stop_reason']}"
    return f"{reason} at step {out['n_iter']}, lowest at {out['nstep']}"


class Reused:
    """One handle ``h = make()`` that runs a chain of solves.  ``link(name, run)`` runs ``run(h)``, then ``run`` on a fresh
    ``make()`` that is closed afterwards, and asks for the same dictionary from both, bit for bit; from the second link on it
    also asks that the solve began somewhere else than the one before it on ``h`` (a pair whose B repeats A shows nothing) and
    prints the pair's REUSE line."""

    def __init__(self, kind, make):
        """``make()``: a new handle, or a list of them (the handles of a shard)."""
        self.kind, self.make = kind, make
        self.h = make()
        self.prev = None
        self.pairs = 0

    def link(self, name, run, compare=True):
        got = run(self.h)
        if compare:
            fresh = self.make()
            try:
                want = run(fresh)
            finally:
                self.close_one(fresh)
            outs = list(zip(got, want)) if isinstance(got, list) else [(got, want)]
            for i, (g, w) in enumerate(outs):
                same_out(g, w, (self.kind, name, i, "reused handle against a fresh one"))
        self.follow(name, got)
        return got

    def follow(self, name, got):
        """Record ``got`` as the solve that ran last on the handle (``None``: an A driven by hand and left unfinished)."""
        if self.prev is not None and got is not None:
            a_name, a = self.prev
            ys = got if isinstance(got, list) else [got]
            xs = a if isinstance(a, list) else [a] * len(ys)
            for i, (x, y) in enumerate(zip(xs, ys)):
                if x is not None:
                    assert first_entries(x) != first_entries(y), (self.kind, a_name, name, i, "B starts where A started", first_entries(y))
                print(f"REUSE {self.kind}{f' [{i}]' if len(ys) > 1 else ''} A = {a_name}: "
                      f"{ending(x) if x is not None else 'left unfinished'} | B = {name}: {ending(y)}")
            self.pairs += 1
        self.prev = (name, got)

    @staticmethod
    def close_one(h):
        for x in h if isinstance(h, list) else [h]:
            x.close()

    def close(self):
        self.close_one(self.h)


def every_ordered_pair(n):
    """A closed walk over 0 .. n - 1 that takes every ordered pair (i, j), i != j, exactly once as a step i -> j: an Euler circuit
    of the complete directed graph (Hierholzer).  n (n - 1) + 1 entries."""
    left = {v: [w for w in range(n) if w != v] for v in range(n)}
    stack, walk = [0], []
    while stack:
        v = stack[-1]
        if left[v]:
            stack.append(left[v].pop())
        else:
            walk.append(stack.pop())
    walk.reverse()
    steps = list(zip(walk, walk[1:]))
    assert len(steps) == n * (n - 1) == len(set(steps)) and all(i != j for i, j in steps), walk
    return walk


def scaled(case, s):
    """``case`` with every scripted value and its tolerance multiplied by ``s``: every ratio the stop rules look at is unchanged, so it
    ends for the case's reason at the case's step -- at another tolerance and on another trace."""
    return case._replace(values=lambda d, m, v=case.values: [s * x for x in v(d, m)], eps=s * case.eps)


def gmres_against_restatement(label, out, t64, t32):
    """A device GMRES adjoint solve that a budget ends against the float64 and the plain-fp32 restatement of the same solve
    (``adjoint_gmres_ref.gmres_adjoint``): the counts of the float64 run, and the result and the last trace entries no further from
    float64 than 16 x the fp32 restatement is, plus 4 ulp -- the gate of tests/test_gpu_adjoint_widths.py::_one_cycle_gate at
    another restart length."""
    eps32 = float(np.finfo(np.float32).eps)

    def rel(a, b):
        a, b = torch.as_tensor(a, dtype=torch.float64).cpu().reshape(-1), torch.as_tensor(b, dtype=torch.float64).cpu().reshape(-1)
        return float((a - b).norm() / b.norm())
    for k in ("n_cycles", "nstep", "stop"):
        assert out[k] == t64[k] == t32[k], (label, k, out[k], t64[k], t32[k])
    assert out["stop"] == "budget", (label, out["stop"])
    assert len(out["rel_trace"]) == len(out["abs_trace"]) == out["n_cycles"], (label, len(out["rel_trace"]))
    assert out["lowest"] == min(out["rel_trace"]), (label, out["lowest"], out["rel_trace"])
    gates = [("result", rel(out["result"], t64["result"]), rel(t32["result"], t64["result"]))]
    for tr in ("rel_trace", "abs_trace"):
        gates.append((tr, rel(out[tr][-1], t64[tr][-1]), rel(t32[tr][-1], t64[tr][-1])))
    print(f"REUSE gmres {label} against the restatement: " + ", ".join(f"{w} e_dev {d:.2e} e32 {p:.2e}" for w, d, p in gates))
    for w, d, p in gates:
        assert d <= 16 * p + 4 * eps32, (label, w, d, p)
