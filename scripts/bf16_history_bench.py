"""fp32 against bf16 storage of the Broyden pairs (``history_dtype``), alternating in one process.  One JSON line per case and
history: seconds, iterations/s, n_iter, stop_reason, lowest, nstep, solver GB; for the threshold-300 and 100k cases also the
achieved bytes/s of the sweep kernels from a profiled repeat, and one "compare" line per case with the two histories' sweep time
over the iterations both ran.

    python scripts/bf16_history_bench.py [--out DIR] [--reps R] [--cases 1m300,1m1500,100k,adjoint]

The profiled repeat polls the stop flag after every iteration (poll_every = 1), so no iteration is issued past the stop, and it
drops the V and U2 sweeps of the final iteration: that iteration's stop test runs between sweep 1 and sweep V, so those two return
at once (their stated bytes were never moved).  Every remaining launch is a sweep that did its work.

Cases: the 1M-node mesh and weights of scripts/big_threshold.py at thresholds 300 and 1 500 (eps 1e-5, as there); a 100k-node
mesh at fw_thres 300, fw_tol 1e-5; the adjoint solve of a 50-graph training batch at bw_tol 1e-8, bw_thres 300."""
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
pkg = importlib.import_module("psi-gnn_amd")
eng = importlib.import_module("psi-gnn_amd.engine")
nat = importlib.import_module("psi-gnn_amd._native")
dev = torch.device("cuda:0")
HIST = {"fp32": torch.float32, "bf16": torch.bfloat16}
PEAK = 8.0e12   # MI355X HBM3E peak, bytes/s


def weights():
    w = np.load(os.path.join(ROOT, "tests", "golden", "weights_dirichlet.npz"))
    return {k: torch.from_numpy(w[k]) for k in w.files}


def fmap_of(mesh, sd):
    md = mesh.to(dev)
    P = "autoencoder.encoder.mlp.mlp."
    h0 = eng.mlp2(md.x, *[sd[P + k].to(dev) for k in ("0.weight", "0.bias", "2.weight", "2.bias")])
    return eng.FixedPointMap(eng.MeshPlan(md), eng.PackedWeights(sd, dev), h0, md.prb_data)


def sweeps_by_iteration(log, n_iter):
    """[(iteration, kernel, ms, bytes)] of the sweep launches that did work.  One `k_reduce_check` per iteration: sweep 1 comes before
    it, sweeps V and U2 after it; those two of the final iteration (n_iter - 1) come after its stop test and return at once."""
    out, it = [], 0
    for name, ms, byts in log:
        if name == "k_reduce_check":
            it += 1
            continue
        if not name.startswith("k_sweep"):
            continue
        if name.startswith("k_sweep_u1"):
            out.append((it, name, ms, byts))
        elif it - 1 < n_iter - 1:
            out.append((it - 1, name, ms, byts))
    return out


def rates(sw):
    agg = {}
    for _, name, ms, byts in sw:
        c, m, b = agg.get(name, (0, 0.0, 0))
        agg[name] = (c + 1, m + ms, b + byts)
    return {k: {"calls": c, "ms": round(m, 3), "GB": round(b / 1e9, 3), "TB_per_s": round(b / (m * 1e-3) / 1e12, 3) if m > 0 else 0.0,
                "of_peak": round(b / (m * 1e-3) / PEAK, 3) if m > 0 else 0.0} for k, (c, m, b) in agg.items()}


def run(case, thr, hd, solve, profile):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out, gb = solve(hd, 50)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    rec = {"case": case, "threshold": thr, "history": hd, "seconds": round(dt, 4), "iters_per_sec": round(out["n_iter"] / dt, 1),
           "n_iter": out["n_iter"], "stop_reason": out["stop_reason"], "lowest": out["lowest"], "nstep": out["nstep"],
           "solver_GB": round(gb, 3)}
    per_it = None
    if profile:
        nat.prof_enable(True)
        nat.prof_collect()
        o2, _ = solve(hd, 1)
        torch.cuda.synchronize()
        nat.prof_collect()
        log = nat.prof_launch_log()
        nat.prof_enable(False)
        sw = sweeps_by_iteration(log, o2["n_iter"])
        rec["sweeps"] = rates(sw)
        per_it = [0.0] * o2["n_iter"]
        for it, _, ms, _ in sw:
            per_it[it] += ms
    return rec, per_it


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=1)
    ap.add_argument("--cases", default="1m300,1m1500,100k,adjoint")
    a = ap.parse_args()
    cases = set(a.cases.split(","))
    sd = weights()
    recs = []

    def emit(r):
        print(json.dumps(r), flush=True)
        recs.append(r)

    def forward_case(name, fm, thr, eps, profile):
        def solve(hd, poll_every):
            sv = eng.DeviceBroyden(plan=fm.plan, threshold=thr, keep_trace=False, history_dtype=HIST[hd])
            try:
                return sv.solve(fm, eps, poll_every=poll_every), sv.nbytes / 1e9
            finally:
                sv.close()
        for _ in range(a.reps):
            per_it = {}
            for hd in ("fp32", "bf16"):
                rec, per_it[hd] = run(name, thr, hd, solve, profile)
                emit(rec)
            if profile:
                # the same iterations (k = 0 .. n - 1 stored pairs) in both histories: the sweeps' time for the pairs, like for like
                n = min(len(per_it["fp32"]), len(per_it["bf16"])) - 1
                t32, t16 = sum(per_it["fp32"][:n]), sum(per_it["bf16"][:n])
                pairs = n * (n - 1) // 2
                emit({"case": name, "threshold": thr, "compare": f"sweep time over iterations 0 .. {n - 1}", "fp32_ms": round(t32, 3),
                      "bf16_ms": round(t16, 3), "fp32_over_bf16": round(t32 / t16, 3), "pair_sweeps": pairs,
                      "fp32_us_per_pair": round(1e3 * t32 / max(pairs, 1), 3), "bf16_us_per_pair": round(1e3 * t16 / max(pairs, 1), 3)})

    if cases & {"1m300", "1m1500"}:
        fm = fmap_of(pkg.data.make_hex_problem(577, seed=0, compute_sol=False), sd)
        if "1m300" in cases:
            forward_case(f"mesh1m_{fm.plan.N}", fm, 300, 1e-5, True)
        if "1m1500" in cases:
            forward_case(f"mesh1m_{fm.plan.N}", fm, 1500, 1e-5, False)
        del fm
        torch.cuda.empty_cache()
    if "100k" in cases:
        fm = fmap_of(pkg.data.make_hex_problem(183, seed=0, compute_sol=False), sd)
        forward_case(f"mesh100k_{fm.plan.N}", fm, 300, 1e-5, True)
        del fm
    if "adjoint" in cases:
        # adjoint solve of a 50-graph training batch (one union batch, as the reference's DataParallel call collates it)
        model = importlib.import_module("psi-gnn_amd.model_psignn")
        collate = importlib.import_module("psi-gnn_amd.data.meshdata").collate
        bt = collate([pkg.data.make_hex_problem(13 + (s % 5), seed=s, compute_sol=False) for s in range(50)]).to(dev)
        for _ in range(a.reps):
            for hd in ("fp32", "bf16"):
                net = model.ModelDEQDSS(dict(latent_dim=10, n_layers=1, fw_tol=1e-5, fw_thres=300, bw_tol=1e-8, bw_thres=300,
                                             broyden_history_dtype=HIST[hd]))
                net.load_state_dict(sd)
                net = net.to(dev)
                with torch.no_grad():
                    h0 = net.autoencoder.encoder(bt.x)
                    hs = net.deqdss(h0, bt)["result"]
                grad = torch.randn(hs.shape, generator=torch.Generator().manual_seed(9)).to(dev)
                net.deqdss.implicit_backward(hs, h0, bt, grad)   # (allocates the kept adjoint solver)

                def solve(_hd, _poll_every):   # (the history is the model's; the adjoint loop polls every 8 iterations)
                    o = net.deqdss.implicit_backward(hs, h0, bt, grad)
                    return o, net.deqdss._bw_solver.nbytes / 1e9
                emit(run(f"adjoint_batch50_{bt.num_nodes}", 300, hd, solve, False)[0])
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "bf16_history_bench.json"), "w") as f:
            json.dump(recs, f, indent=1)


if __name__ == "__main__":
    main()
