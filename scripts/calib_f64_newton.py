"""Where the gates of tests/test_gpu_f64_newton.py come from: the float64 restatement of the shifted linear solve
(tests/newton64_ref.py, ``gmres_shifted`` on the float64 oracle's autograd products) against itself with the oracle's edge list
permuted, three seeds -- the summation order is the only freedom a correct float64 statement has.  Per case (two stored fixtures
and a random two-layer block of each family, at the stored ``fp64_result``), shift (1.0, 1.5) and orientation (J, J^T), with
eta 1e-2, m 50, budget 200 and b = randn (seed ``B_SEED``): whether products, cycles, stop reason and n_reorth agree between the
runs, and how far the result moves (relative L2).  Then the duality check: both orientations to eta 1e-12 at shift 1.5 (budget
2000); <w, d_forward(b)> and <d_transposed(w), b> differ by <r_t, d_f> - <d_t, r_f>, so the figure is
|a - c| / (|w| |d_f| + |d_t| |b|), for the stored edge order and every permuted one.  CPU only:

    python scripts/calib_f64_newton.py [seed of b ...]
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import newton64_ref as ref   # noqa: E402
from train_step_ref import permuted   # noqa: E402

PERM_SEEDS = (1, 2, 3)


def rel(a, b):
    return float((a - b).norm() / b.norm())


def counts(o):
    return o["nstep"], o["n_cycles"], o["stop"], o["n_reorth"]


def duality(p):
    f = p.solve(1.5, False, eta=1e-12, max_products=2000)
    t = p.solve(1.5, True, eta=1e-12, max_products=2000, b=p.w)
    a, c = float((p.w * f["result"]).sum()), float((t["result"] * p.b).sum())
    scale = float(p.w.norm() * f["result"].norm() + t["result"].norm() * p.b.norm())
    return a, c, abs(a - c) / scale, f, t


def run(name, b_seed):
    base = ref.LinearProblem(name, seed=b_seed)
    perms = [ref.LinearProblem(name, mesh=permuted(base.mesh, [], s, False)[0], seed=b_seed) for s in PERM_SEEDS]
    worst, all_equal = 0.0, True
    for shift in ref.SHIFTS:
        for transposed in (False, True):
            o = base.solve(shift, transposed)
            moved, same = [], []
            for q in perms:
                oq = q.solve(shift, transposed)
                same.append(counts(oq) == counts(o))
                moved.append(rel(oq["result"], o["result"]))
            worst = max(worst, *moved)
            all_equal &= all(same)
            print(f"{name:22s} shift {shift} {'J^T' if transposed else 'J  '}: products/cycles/stop/n_reorth {counts(o)} "
                  f"lowest {o['lowest']:.3e}; permuted: counts equal {same}, result moved {max(moved):.2e}")
    a, c, gap, f, t = duality(base)
    gaps, da = [gap], []
    for q in perms:
        aq, cq, gq, _, _ = duality(q)
        gaps.append(gq)
        da.append(max(abs(aq - a), abs(cq - c)) / max(abs(a), 1e-300))
    print(f"{name:22s} duality at shift 1.5, eta 1e-12: <w, d_f> {a:.15e} <d_t, b> {c:.15e}; products {f['nstep']} / {t['nstep']} "
          f"stops {f['stop']} / {t['stop']}; normalised gap {gap:.2e} (permuted: {', '.join(f'{g:.2e}' for g in gaps[1:])}); "
          f"the products themselves moved <= {max(da):.2e} relative")
    return worst, all_equal, max(gaps)


def main():
    seeds = [int(a) for a in sys.argv[1:]] or [ref.B_SEED]
    for b_seed in seeds:
        print(f"---- b = randn, seed {b_seed}")
        res = [run(name, b_seed) for name in ref.CASE_NAMES]
        w, g = max(r[0] for r in res), max(r[2] for r in res)
        print(f"seed {b_seed}: counts agree on every case: {all(r[1] for r in res)}; worst result movement {w:.2e} -> gate 250 x = "
              f"{250 * w:.2e}; worst normalised duality gap {g:.2e} -> gate 250 x = {250 * g:.2e}")


if __name__ == "__main__":
    main()
