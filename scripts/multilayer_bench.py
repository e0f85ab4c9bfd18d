"""Derivatives of an L-layer dirichlet block at 1M nodes, L = 1, 2, 3: one JSON line.

Median HIP-event times (after one warm call) of the plan-order VJP (fmap.vjp_p: the stateless form, which evaluates the layer
states h_1..h_{L-1} first), the plan-order JVP (fmap.jvp_p, likewise) and one adjoint-solve iteration (a device Broyden solve
of y = J^T y + g at a fixed state with eps = 0, so that it runs its whole budget; the layer states are evaluated once per
solve, each iteration then runs the L backward layers).  Weights: the trained checkpoint's layer 0 stacked into every layer.
Also the parameter VJP with the h_initial cotangent (fmap.param_vjp_init, caller's numbering) and the backward of the VJP
(fmap.vjp_backward, caller's numbering, global-gather kernels).
    python scripts/multilayer_bench.py [--reps 30] [--iters 40] [--out file.json] [--layers 1 2 3]"""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("psi-gnn_amd")
eng = importlib.import_module("psi-gnn_amd.engine")
mp = importlib.import_module("psi-gnn_amd.model_psignn")
dev = torch.device("cuda:0")


def weights(L):
    w = np.load(os.path.join(ROOT, "tests", "golden", "weights_dirichlet.npz"))
    sd = {k: torch.from_numpy(w[k]) for k in w.files}
    for k in list(sd):
        for mod in ("phi_to_list", "phi_from_list", "update_list"):
            if f".f.{mod}.0." in k:
                for l in range(1, L):
                    sd[k.replace(f"{mod}.0.", f"{mod}.{l}.")] = sd[k].clone()
    return sd


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(ts))


def run(mesh, L, reps, iters):
    net = mp.ModelPSIGNN(dict(latent_dim=10, n_layers=L))
    net.load_state_dict(weights(L))
    net = net.to(dev).eval()
    with torch.no_grad():
        h0 = net.autoencoder.encoder(mesh.x)
    fm = net.deqdss.f.bind(h0, mesh)
    Hp = fm.to_plan(fm.h0)
    for _ in range(10):   # a state along the forward iteration (Dirichlet rows = h_initial's), not the encoder output
        Hp = fm.fp(Hp)
    g = torch.Generator(device=dev).manual_seed(1)
    Wp, Vp = torch.randn(Hp.shape, device=dev, generator=g), torch.randn(Hp.shape, device=dev, generator=g)
    r = {"L": L, "N": int(fm.plan.N), "Ep": int(fm.plan.Ep)}
    r["vjp_p_us"] = timed(lambda: fm.vjp_p(Hp, Wp), reps)
    r["jvp_p_us"] = timed(lambda: fm.jvp_p(Hp, Vp), reps)
    H = fm.from_plan(Hp)
    W_, V_ = fm.from_plan(Wp), fm.from_plan(Vp)
    r["param_vjp_us"] = timed(lambda: fm.param_vjp_init(H, W_), reps)
    r["vjp_backward_us"] = timed(lambda: fm.vjp_backward(H, W_, V_), max(3, reps // 3))
    sv = eng.DeviceBroyden(plan=fm.plan, threshold=iters, keep_trace=False)
    try:
        grad = fm.from_plan(Wp)
        sv.solve_adjoint(fm, H, grad, 0.0)   # buffers
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        o = sv.solve_adjoint(fm, H, grad, 0.0)
        e1.record()
        e1.synchronize()
        r["adjoint_solve_ms"] = e0.elapsed_time(e1)
        r["adjoint_iters"] = int(o["n_iter"])
        r["adjoint_us_per_iter"] = r["adjoint_solve_ms"] * 1e3 / max(1, int(o["n_iter"]))
    finally:
        sv.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--layers", type=int, nargs="+", default=[1, 2, 3])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = pkg.data.hex_n_for_nodes(1_000_000)
    mesh = pkg.data.make_hex_problem(n, seed=0, compute_sol=False).to(dev)
    res = {"device": torch.cuda.get_device_name(0), "timing": "median of HIP-event pairs around one call, after one warm call",
           "rows": [run(mesh, L, a.reps, a.iters) for L in a.layers]}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
