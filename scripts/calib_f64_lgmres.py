"""Where the gates of tests/test_gpu_f64_lgmres.py come from: the float64 restatement of the augmented GMRES
(tests/lgmres_ref.py) against itself under a rounding-level perturbation of every product -- each product of the float64 oracle is
multiplied, element by element, by 1 + s * 2^-52 with s uniform in [-4, 4] (three seeds), the freedom a correct float64 statement
with another summation order has (the rule of scripts/calib_f64_adjoint.py).  The runs are those of the GPU tests:

* test 2: the three fixtures, m 10, augment 1 / 2, stall 1.0, eps 1e-10, budget 60 (seven cycles, the last with left = 4);
* test 4: the shifted system on hex13_dirichlet_s0, m 8, augment 2, stall 1.0, eta 1e-8, shift 1.0 / 1.5, both orientations;
* test 5: line graphs of 1, 51, 52, 103 and 129 nodes, m 4, augment 3, budgets 5 c + 2 and 5 c + 3, c = 1, 2, 3 (cycle c is the last,
  with left = 1 and 2).

Prints, per run, whether a count moved and how far the result and the trace entries moved, and the worst of each group.  CPU only:

    python scripts/calib_f64_lgmres.py
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import adjoint_gmres_ref as ref   # noqa: E402
import lgmres_ref as lg   # noqa: E402
import newton64_ref as nref   # noqa: E402
import vjp_backward_cases as vb   # noqa: E402
from conftest import load_weights   # noqa: E402
from oracle import psignn_oracle as orc   # noqa: E402

COUNTS = ("nstep", "n_cycles", "n_aug", "stop", "n_reorth")
LINE_NODES = (1, 51, 52, 103, 129)
LINE_BUDGETS = tuple(5 * c + 1 + left for c in (1, 2, 3) for left in (1, 2))   # cycle c is the last, with `left` steps


def perturbed(op, seed):
    gen = torch.Generator().manual_seed(seed)

    def f(w):
        out = op(w)
        s = torch.rand(out.shape, generator=gen, dtype=torch.float64) * 8.0 - 4.0
        return out * (1.0 + s * 2.0 ** -52)
    return f


def spread(what, solve, op, seeds=(1, 2, 3)):
    """``solve(op)``: one run of the restatement.  Returns (a count moved, result moved, trace moved abs, trace moved rel)."""
    base = solve(op)
    moved, dres, dabs, drel = False, 0.0, 0.0, 0.0
    for seed in seeds:
        o = solve(perturbed(op, seed))
        same = all(o[k] == base[k] for k in COUNTS)
        moved |= not same
        scale = float(base["result"].norm())
        dres = max(dres, float((o["result"] - base["result"]).norm()) / scale if scale else 0.0)
        n = min(len(o["rel_trace"]), len(base["rel_trace"]))
        for tr in ("rel_trace", "abs_trace"):
            for a, b in zip(o[tr][:n], base[tr][:n]):
                dabs = max(dabs, abs(a - b))
                drel = max(drel, abs(a - b) / b if b else 0.0)
    print(f"{what}: {' / '.join(str(base[k]) for k in COUNTS)} lowest {base['lowest']:.3e}; a count moved: {moved}; result moved "
          f"<= {dres:.2e}; trace entries moved <= {dabs:.1e} abs, {drel:.1e} rel", flush=True)
    return moved, dres, dabs, drel


def worst(name, rows):
    print(f"== {name}: a count moved in {sum(r[0] for r in rows)} of {len(rows)} runs; result moved <= {max(r[1] for r in rows):.2e}; "
          f"trace entries moved <= {max(r[2] for r in rows):.1e} abs, {max(r[3] for r in rows):.1e} rel; 250 x the result's: "
          f"{250 * max(r[1] for r in rows):.2e}, 250 x the traces' rel: {250 * max(r[3] for r in rows):.2e}", flush=True)


def line_problem(N, mixed=False):
    """The adjoint system of a line graph at the encoder state on the float64 oracle: (vjp, grad)."""
    mesh = vb.line_graph(N, mixed)
    s64, m64 = vb.to64(load_weights("mixed" if mixed else "dirichlet"), mesh)
    with torch.no_grad():
        h0 = orc.encoder(s64, m64.x)
    hh = h0.clone().requires_grad_(True)
    out = orc.function_forward(s64, hh, h0, m64)
    grad = torch.randn(h0.shape, generator=torch.Generator().manual_seed(N), dtype=torch.float64)
    return (lambda w: torch.autograd.grad(out, hh, w, retain_graph=True)[0]), grad


def main():
    rows = []
    for name in ref.FIXTURES:
        p = ref.AdjointProblem(name)
        g64 = p.grad.double()
        for augment in (1, 2):
            rows.append(spread(f"{name} m 10 augment {augment} budget 60",
                               lambda op, a=augment: lg.lgmres_adjoint(op, g64, 1e-10, 60, m=10, augment=a, stall=1.0), p.vjp64))
    worst("test 2", rows)
    rows = []
    lp = nref.LinearProblem("hex13_dirichlet_s0")
    for shift in nref.SHIFTS:
        for transposed in (False, True):
            rows.append(spread(f"shifted, shift {shift} {'J^T' if transposed else 'J'} m 8 augment 2 eta 1e-8",
                               lambda op, s=shift: lg.lgmres_adjoint(op, lp.b, 1e-8, 200, m=8, augment=2, stall=1.0, shift=s, lin=True),
                               lp.op(transposed)))
    worst("test 4", rows)
    rows = []
    for N in LINE_NODES:
        vjp, grad = line_problem(N)
        for budget in LINE_BUDGETS:
            rows.append(spread(f"line{N} m 4 augment 3 budget {budget}",
                               lambda op, b=budget: lg.lgmres_adjoint(op, grad, 1e-10, b, m=4, augment=3, stall=1.0), vjp))
    worst("test 5", rows)


if __name__ == "__main__":
    main()
