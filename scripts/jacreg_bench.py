"""Backward of the VJP (csrc/gather_backward.hip; its tile form csrc/fgnn_tile_jr.hip) on one large mesh or one union batch:
time per call, per-kernel breakdown.

    python3 scripts/jacreg_bench.py [hex_n=577] [reps=10] [--route gather|tiled|both] [--union B] [--warmup W] [--out FILE]

``--route gather`` (default) times ``fmap.vjp_backward`` as before; ``tiled`` times ``fmap.vjp_backward(..., tiled=True)``;
``both`` times the two routes alternately, call by call, in this process on the same inputs (every call between two device
synchronisations, W warm-up calls per route first) and reports median and min - max of each, then each route's kernels from a
profiled pass of its own.  ``--union B``: a union batch of B hexagon meshes of size hex_n (seeds 0..B-1) instead of one mesh.
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = lambda n="": importlib.import_module("psi-gnn_amd" + ("." + n if n else ""))

HBM_PEAK = 8.0e12   # bytes / s (MI355X)


def _kernels(nat, call, reps):
    """Per-kernel averages (us) and algorithmic bytes of ``reps`` profiled calls."""
    nat.prof_enable(True)
    nat.prof_collect()
    for _ in range(reps):
        call()
    torch.cuda.synchronize()
    kern = nat.prof_collect(with_bytes=True)
    nat.prof_enable(False)
    out = {}
    for k, v in sorted(kern.items(), key=lambda kv: -kv[1][1]):
        us = 1e3 * v[1] / v[0]
        out[k] = {"us": round(us, 1), "launches_per_call": v[0] / reps}
        if len(v) > 2 and v[2]:
            bpl = v[2] / v[0]
            out[k].update(bytes=int(bpl), hbm_fraction=round(bpl / (us * 1e-6) / HBM_PEAK, 3))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("hex_n", nargs="?", type=int, default=577)
    ap.add_argument("reps", nargs="?", type=int, default=10)
    ap.add_argument("--route", choices=("gather", "tiled", "both"), default="gather")
    ap.add_argument("--union", type=int, default=0)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, reps = a.hex_n, a.reps
    data, nat, eng = pkg("data"), pkg("_native"), pkg("engine")
    w = np.load(os.path.join(ROOT, "tests", "golden", "weights_dirichlet.npz"))
    sd = {k: torch.from_numpy(w[k]) for k in w.files}
    dev = torch.device("cuda:0")
    if a.union:
        mesh = data.collate([data.make_hex_problem(n, seed=s, compute_sol=False) for s in range(a.union)]).to(dev)
        what = f"union batch of {a.union} hexagon meshes n={n}"
    else:
        mesh = data.make_hex_problem(n, seed=0).to(dev)
        what = f"hexagon n={n}"
    W = eng.PackedWeights(sd, dev)
    enc = pkg("model_psignn").ModelDEQDSS(dict(latent_dim=10, n_layers=1))
    enc.load_state_dict(sd)
    h0 = enc.to(dev).autoencoder.encoder(mesh.x).detach()
    fmap = eng.FixedPointMap(eng.plan_for(mesh), W, h0, mesh.prb_data, None)
    h = fmap(fmap(h0))
    v = torch.randn(h.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    g = fmap.vjp(h, v)
    gbar = 2.0 * g / h.numel()
    N = h.shape[0]
    calls = {"gather": lambda: fmap.vjp_backward(h, v, gbar), "tiled": lambda: fmap.vjp_backward(h, v, gbar, tiled=True)}
    res = {"workload": f"backward of the VJP, {what}: {N} nodes", "record_bytes": 2 * N * 320 * 4,
           "jac_loss": float(g.norm() ** 2 / h.numel())}
    if a.route != "both":
        call = calls[a.route]
        call()
        torch.cuda.synchronize()
        nat.prof_enable(True)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            grads, dh = call()
        e1.record()
        torch.cuda.synchronize()
        kern = nat.prof_collect()
        nat.prof_enable(False)
        res.update(route=a.route, ms_per_call=e0.elapsed_time(e1) / reps,
                   kernels_us={k: round(1e3 * v[1] / v[0], 1) for k, v in sorted(kern.items(), key=lambda kv: -kv[1][1])},
                   grad_norm=float(torch.cat([t.reshape(-1) for t in grads.values()]).norm()))
    else:
        routes = ("gather", "tiled")
        for r in routes:
            for _ in range(max(a.warmup, 1)):
                out = calls[r]()
        torch.cuda.synchronize()
        ms = {r: [] for r in routes}
        for _ in range(reps):
            for r in routes:     # alternated call by call
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                calls[r]()
                torch.cuda.synchronize()
                ms[r].append(1e3 * (time.perf_counter() - t0))
        for r in routes:
            t = np.array(ms[r])
            res[r] = {"calls": len(t), "warmup": max(a.warmup, 1), "median_ms": float(np.median(t)), "min_ms": float(t.min()),
                      "max_ms": float(t.max())}
        res["tiled_over_gather_median"] = res["tiled"]["median_ms"] / res["gather"]["median_ms"]
        # the timed calls include the permutations of the caller-order entry (tiled: three in, one out); the plan-order entry alone:
        Hp, Vp, Gp = fmap.to_plan(h), fmap.to_plan(v), fmap.to_plan(gbar)
        for _ in range(max(a.warmup, 1)):
            fmap.vjp_backward_p(Hp, Vp, Gp)
        t = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fmap.vjp_backward_p(Hp, Vp, Gp)
            torch.cuda.synchronize()
            t.append(1e3 * (time.perf_counter() - t0))
        res["tiled_plan_order"] = {"calls": reps, "median_ms": float(np.median(t)), "min_ms": float(min(t)), "max_ms": float(max(t))}
        for r in routes:
            res[r]["kernels"] = _kernels(nat, calls[r], 5)
        gg, dg = calls["gather"]()
        gt, dt = calls["tiled"]()
        sc = max(float(t.norm()) for t in gg.values())
        res["routes_differ_by"] = {"worst_tensor": max(float((gt[k] - gg[k]).norm()) / max(float(gg[k].norm()), 1e-4 * sc) for k in gg),
                                   "dh": float((dt - dg).norm() / dg.norm())}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
