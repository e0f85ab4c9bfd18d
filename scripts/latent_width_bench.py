"""Forward inference at latent widths 8, 10 and 16 on the 1 000 519-node bench mesh: one JSON line per width.

Mesh: bench.py's ``mesh1m`` recipe (make_hex_problem(hex_n_for_nodes(1e6), seed=0)); weights: seeded random blocks
(torch.manual_seed(5), normal_(std=0.1) on the 1-D parameters) at every width, so that the three widths run the same kind of
problem; K = 20 stored pairs.  The widths alternate inside every region (a b c a b c ...), five regions, medians:
    plain f          HIP-event time of fmap.fp (k_f_tile), REPS calls per region
    fused step       k_f_tile_fused per launch, from the library's launch records of a K-iteration Broyden solve
    Broyden iteration  event time of that solve / its iterations (records off)
each with its algorithmic bytes (as the launch sites state them) and the fraction of the 8 TB/s HBM peak.
    python scripts/latent_width_bench.py [--out FILE] [--widths 8,10,16] [--default-lib PATH] [--nodes N]
--default-lib: run width 10 on another build of libpsignn_hip.so (the parent commit's, for the before / after yardstick); a build
that predates ``psignn_latent_dim`` is accepted.  --quick: one region, for a run under rocprofv3 --kernel-trace --stats."""
import argparse
import ctypes
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("psi-gnn_amd")
nat = importlib.import_module("psi-gnn_amd._native")
eng = importlib.import_module("psi-gnn_amd.engine")
mp = importlib.import_module("psi-gnn_amd.model_psignn")
solver = importlib.import_module("psi-gnn_amd.utilities.solver")
dev = torch.device("cuda:0")
PEAK = 8e12
K = 20


def use_default_lib(path):
    """Bind another build of the default-width library (every name of SIGNATURES it exports) in place of the tree's."""
    l = ctypes.CDLL(path)
    for name, (res, args) in nat.SIGNATURES.items():
        if hasattr(l, name):
            fn = getattr(l, name)
            fn.restype, fn.argtypes = res, args
    l.width = nat.D
    nat._libs[nat.D] = l


def event_us(fn, reps=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def make(d, mesh):
    torch.manual_seed(5)
    net = mp.ModelPSIGNN(dict(latent_dim=d, n_layers=1))
    for p in net.parameters():
        if p.dim() == 1:
            torch.nn.init.normal_(p, std=0.1)
    net = net.to(dev).eval()
    with torch.no_grad():
        h0 = net.autoencoder.encoder(mesh.x)
    fm = net.deqdss.f.bind(h0, mesh)
    sv = eng.DeviceBroyden(plan=fm.plan, threshold=K, keep_trace=False, width=d)
    return {"d": d, "fm": fm, "sv": sv, "xp": fm.to_plan(fm.h0), "f": [], "fused": [], "iter": [], "bytes": {}}


def region(c, reps):
    fm, sv, d = c["fm"], c["sv"], c["d"]
    c["f"].append(event_us(lambda: fm.fp(c["xp"]), reps))
    out = {}
    t = event_us(lambda: out.update(sv.solve(fm, 1e-30)))
    c["iter"].append(t / max(out["n_iter"], 1))
    c["n_iter"] = out["n_iter"]
    nat.prof_enable(True, width=d)
    nat.prof_collect(width=d)
    fm.fp(c["xp"])
    sv.solve(fm, 1e-30)
    rec = nat.prof_collect(with_bytes=True, width=d)
    nat.prof_enable(False, width=d)
    calls, ms, byts = rec["k_f_tile_fused"]
    c["fused"].append(ms * 1e3 / calls)
    c["bytes"] = {"f": rec["k_f_tile"][2] // rec["k_f_tile"][0], "fused": byts // calls,
                  "iteration": sum(v[2] for k, v in rec.items() if k != "k_f_tile") // max(c["n_iter"], 1)}
    c["kernels"] = sorted(rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--widths", default="8,10,16")
    ap.add_argument("--default-lib")
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    if a.default_lib:
        use_default_lib(a.default_lib)
    mesh = pkg.data.make_hex_problem(pkg.data.hex_n_for_nodes(a.nodes), seed=0, compute_sol=False).to(dev)
    cases = [make(int(w), mesh) for w in a.widths.split(",")]
    for c in cases:   # warm: plan-order inputs, solver state, code objects
        c["fm"].fp(c["xp"])
        c["sv"].solve(c["fm"], 1e-30)
    for _ in range(1 if a.quick else 5):
        for c in cases:
            region(c, a.reps)
    lines = []
    for c in cases:
        med = lambda v: float(np.median(v))
        row = {"latent_dim": c["d"], "N": int(c["fm"].plan.N), "Ep": int(c["fm"].plan.Ep), "K": K, "n_iter": c["n_iter"],
               "library": "--default-lib " + os.path.basename(a.default_lib) if (a.default_lib and c["d"] == nat.D)
               else os.path.basename(nat.lib_path(c["d"])), "kernels": c["kernels"]}
        for key, ts in (("f", c["f"]), ("fused", c["fused"]), ("iteration", c["iter"])):
            us = med(ts)
            row[key + "_us"] = round(us, 2)
            row[key + "_us_regions"] = [round(t, 2) for t in ts]
            row[key + "_bytes"] = int(c["bytes"][key])
            row[key + "_frac_of_8TBps"] = round(c["bytes"][key] / (us * 1e-6) / PEAK, 4)
        lines.append(json.dumps(row))
        c["sv"].close()
    print("\n".join(lines))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
