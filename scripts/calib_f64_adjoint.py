"""Where the gates of tests/test_gpu_f64_adjoint.py come from: the float64 CPU oracle's adjoint solves under a rounding-level
perturbation of every product.  Each product of the float64 oracle VJP is multiplied, element by element, by 1 + s * 2^-52 with s
uniform in [-4, 4] (three seeds) -- the freedom a correct float64 statement with another summation order has -- and the float64
GMRES restatement (eps 1e-11, m 50, budget 2000) and the oracle's Broyden under a float64 default dtype (eps 1e-11, threshold
800) are run again.  Prints, per fixture, how far counts, traces, `lowest` and results move.  CPU only:

    python scripts/calib_f64_adjoint.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import adjoint_gmres_ref as ref   # noqa: E402
from oracle import psignn_oracle as orc   # noqa: E402


def perturbed(vjp, seed):
    gen = torch.Generator().manual_seed(seed)

    def f(w):
        out = vjp(w)
        s = torch.rand(out.shape, generator=gen, dtype=torch.float64) * 8.0 - 4.0
        return out * (1.0 + s * 2.0 ** -52)
    return f


def broyden64(vjp, grad, eps=1e-11, threshold=800):
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        with torch.no_grad():
            out = orc.broyden(lambda y: vjp(y) + grad, torch.zeros_like(grad), threshold=threshold, eps=eps)
    finally:
        torch.set_default_dtype(old)
    out["n_iter"] = len(out["xest_trace"]) - 1
    return out


def rel(a, b):
    return float((a - b).norm() / b.norm())


def residual(vjp, grad, y):
    f = vjp(y) + grad
    return float((f - y).norm()) / (float(f.norm()) + 1e-9)


def run(name, p, seeds=(1, 2, 3), traces=True):
    g64 = p.grad.double()
    truth = p.truth()
    base = ref.gmres_adjoint(p.vjp64, g64, 1e-11, 2000, m=50)
    print(f"{name}: GMRES products {base['nstep']} cycles {base['n_cycles']} stop {base['stop']} n_reorth {base['n_reorth']} "
          f"lowest {base['lowest']:.3e} distance to truth {rel(base['result'], truth):.2e}")
    bb = broyden64(p.vjp64, g64)
    print(f"{name}: Broyden steps {bb['n_iter']} lowest {bb['lowest']:.3e} prot_break {bb['prot_break']} "
          f"distance to truth {rel(bb['result'], truth):.2e} residual of the result {residual(p.vjp64, g64, bb['result']):.3e}")
    for seed in seeds:
        o = ref.gmres_adjoint(perturbed(p.vjp64, seed), g64, 1e-11, 2000, m=50)
        same = (o["nstep"], o["n_cycles"], o["stop"]) == (base["nstep"], base["n_cycles"], base["stop"])
        n = min(len(o["rel_trace"]), len(base["rel_trace"]))
        dabs = max(abs(a - b) for tr in ("rel_trace", "abs_trace") for a, b in zip(o[tr][:n], base[tr][:n]))
        drel = max(abs(a - b) / b for tr in ("rel_trace", "abs_trace") for a, b in zip(o[tr][:n], base[tr][:n]))
        res = residual(p.vjp64, g64, o["result"])
        print(f"  seed {seed} GMRES: counts equal {same} ({o['nstep']}, {o['n_cycles']}, {o['stop']}) n_reorth {o['n_reorth']} "
              f"result moved {rel(o['result'], base['result']):.2e} trace entries moved <= {dabs:.1e} abs, {drel:.1e} rel; "
              f"lowest {o['lowest']:.6e} vs true residual {res:.6e} ({abs(o['lowest'] - res) / res:.1e} rel)")
        b = broyden64(perturbed(p.vjp64, seed), g64)
        res = residual(p.vjp64, g64, b["result"])
        line = (f"  seed {seed} Broyden: steps {b['n_iter']} lowest {b['lowest']:.6e} vs true residual {res:.6e} "
                f"({abs(b['lowest'] - res) / res:.1e} rel) prot_break {b['prot_break']} distance to truth {rel(b['result'], truth):.2e}")
        if traces:
            mv = [max(abs(b[tr][i] - bb[tr][i]) / bb[tr][i] for tr in ("rel_trace", "abs_trace"))
                  for i in range(min(b["n_iter"], bb["n_iter"]))]
            first = next((i for i, v in enumerate(mv) if v > 1e-10), None)
            line += f"; entries 0-9 moved <= {max(mv[:10]):.1e} rel, first entry to move by more than 1e-10: {first}"
        print(line)


def main():
    for name in ref.FIXTURES:
        run(name, ref.AdjointProblem(name))
    run("hex13 two layers", ref.AdjointProblem("hex13_dirichlet_s0", sd=ref.stacked_dirichlet(2)), traces=False)


if __name__ == "__main__":
    main()
