"""Where the result gate of tests/test_gpu_adjoint_lgmres.py (check 4) comes from: the fp32 restatement of the augmented GMRES
adjoint solve (tests/lgmres_ref.py on ``AdjointProblem.vjp32``, fp32 vectors) against itself under a rounding-level perturbation of
every product -- each product of the float32 oracle is multiplied, element by element, by 1 + s * 2^-23 with s uniform in [-4, 4]
(three seeds), the freedom a correct fp32 statement with another summation order has (the procedure of
scripts/calib_f64_lgmres.py at fp32's unit).  The runs are those of the GPU test: the three fixtures, m 10, eps 1e-5, budget 800,
(augment, stall) in (0, 0.5), (0, 1.0), (1, 1.0), (2, 1.0); and, at the launch tolerance, eps 1e-8, budget 500, (0, 0.5), (0, 1.0),
(1, 1.0) with the error to ``truth()``.

Prints, per run, the counts, whether a count moved and how far the result moved, and the worst over the runs that ended on
"tolerance" (the runs check 4 compares results on).  CPU only:

    python scripts/calib_adjoint_lgmres.py
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import adjoint_gmres_ref as ref   # noqa: E402
import lgmres_ref as lg   # noqa: E402

COUNTS = ("nstep", "n_cycles", "n_aug", "stop")
OPTS = ((0, 0.5), (0, 1.0), (1, 1.0), (2, 1.0))


def perturbed(op, seed):
    gen = torch.Generator().manual_seed(seed)

    def f(w):
        out = op(w)
        s = torch.rand(out.shape, generator=gen, dtype=torch.float32) * 8.0 - 4.0
        return out * (1.0 + s * 2.0 ** -23)
    return f


def spread(what, solve, op, seeds=(1, 2, 3)):
    """``solve(op)``: one run of the restatement.  Returns (stop, a count moved, result moved, base dict)."""
    base = solve(op)
    moved, dres = False, 0.0
    for seed in seeds:
        o = solve(perturbed(op, seed))
        moved |= not all(o[k] == base[k] for k in COUNTS)
        scale = float(base["result"].double().norm())
        dres = max(dres, float((o["result"].double() - base["result"].double()).norm()) / scale if scale else 0.0)
    print(f"{what}: {' / '.join(str(base[k]) for k in COUNTS)} n_reorth {base['n_reorth']} lowest {base['lowest']:.3e}; a count moved: "
          f"{moved}; result moved <= {dres:.2e}", flush=True)
    return base["stop"], moved, dres, base


def main():
    rows = []
    for name in ref.FIXTURES:
        p = ref.AdjointProblem(name)
        for augment, stall in OPTS:
            row = spread(f"{name} m 10 eps 1e-5 budget 800 augment {augment} stall {stall}",
                         lambda op, a=augment, s=stall: lg.lgmres_adjoint(op, p.grad, 1e-5, 800, m=10, augment=a, stall=s), p.vjp32)
            print(f"    error to truth() {p.error(row[3]['result']):.2e}", flush=True)
            rows.append(row)
        for augment, stall in OPTS[:3]:
            out = lg.lgmres_adjoint(p.vjp32, p.grad, 1e-8, 500, m=10, augment=augment, stall=stall)
            print(f"{name} m 10 eps 1e-8 budget 500 augment {augment} stall {stall}: {' / '.join(str(out[k]) for k in COUNTS)} lowest "
                  f"{out['lowest']:.3e} error to truth() {p.error(out['result']):.2e}", flush=True)
    tol = [r for r in rows if r[0] == "tolerance"]
    print(f"== runs that ended on tolerance: a count moved in {sum(r[1] for r in tol)} of {len(tol)}; result moved <= "
          f"{max(r[2] for r in tol):.2e}; 250 x that: {250 * max(r[2] for r in tol):.2e}", flush=True)


if __name__ == "__main__":
    main()
