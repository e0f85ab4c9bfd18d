"""Anderson / Picard over a shard of R meshes: the lockstep solve (``utilities.solver.anderson_batch`` / ``forward_iteration_batch``)
against the same meshes solved one after the other with ``utilities.solver.anderson`` / ``forward_iteration`` (the route every
shard takes without ``fp_lockstep``), alternated in one process.

    python3 scripts/fpiter_batch_bench.py R n_hex [dirichlet|mixed] [anderson|picard] [repeats=15]

R and n_hex may be comma-separated lists (``1,2,4,8 13,58``): one process then measures every combination.  Each mesh is
``make_hex_problem(n_hex, seed=s)`` on the stored checkpoint; threshold 50, eps 1e-5 (no mesh converges that far in 50 passes, so
every solve does the full 48 / 51 passes and the two routes do the same work).  Prints one JSON line per combination and stores it
in profiles/fpiter_batch_bench.json: median wall seconds per shard solve of either route (host clock around a device synchronise,
handles created and freed inside the solve as a caller sees it), their ratio, whether the results are bit-identical (they are while
the shard stays below the 786 432-element switch to 16 floats per lane; above it the lockstep handles reduce in other block shapes),
and from the library's launch record the recorded launches per pass of either route (the copies of k_fp_copy are not recorded in
either: one gated copy per pass in the lockstep route, per mesh in the sequential one)."""
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = lambda n="": importlib.import_module("psi-gnn_amd" + ("." + n if n else ""))
T, EPS = 50, 1e-5


def measure(R, n, mixed, which, reps, dev, net):
    data, slv, nat = pkg("data"), pkg("utilities.solver"), pkg("_native")
    mds = [data.make_hex_problem(n, seed=s, mixed=mixed, compute_sol=False).to(dev) for s in range(R)]
    with torch.no_grad():
        fmaps = [net.deqdss.f.bind(net.autoencoder.encoder(md.x), md) for md in mds]
    if which == "anderson":
        routes = {"lockstep": lambda: slv.anderson_batch(fmaps, threshold=T, eps=EPS),
                  "sequential": lambda: [slv.anderson(f, f.h0, threshold=T, eps=EPS, keep_trace=False) for f in fmaps]}
        passes = T - 2
    else:
        routes = {"lockstep": lambda: slv.forward_iteration_batch(fmaps, eps=EPS, threshold=T),
                  "sequential": lambda: [slv.forward_iteration(f, f.h0, eps=EPS, threshold=T, keep_trace=False) for f in fmaps]}
        passes = T + 1
    outs = {k: f() for k, f in routes.items()}   # warm-up of every shape the timed window uses
    torch.cuda.synchronize()
    pairs = list(zip(outs["lockstep"], outs["sequential"]))
    same = all(torch.equal(x["result"], y["result"]) and x["nstep"] == y["nstep"] for x, y in pairs)
    diff = max(float((x["result"] - y["result"]).norm() / y["result"].norm()) for x, y in pairs)
    times = {k: [] for k in routes}
    for _ in range(reps):
        for k, f in routes.items():
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t0)
    nat.prof_enable(True)
    recs = {}
    for k, f in routes.items():
        nat.prof_collect()
        f()
        torch.cuda.synchronize()
        recs[k] = {name: v[0] for name, v in nat.prof_collect().items()}
    nat.prof_enable(False)
    med = {k: statistics.median(v) for k, v in times.items()}
    family = "mixed" if mixed else "dirichlet"
    return {"workload": f"{which} ({family} family), shard of {R} hexagon meshes (n={n}): {fmaps[0].plan.N} nodes each; threshold {T}, "
                        f"eps {EPS}, {passes} passes per mesh",
            "family": family, "solver": which, "meshes": R, "n_hex": n, "nodes_per_mesh": fmaps[0].plan.N, "passes": passes,
            "shard_elems": sum(f.plan.N for f in fmaps) * 10, "bit_identical": same, "max_rel_difference": diff,
            "s_median": med, "s_min": {k: min(v) for k, v in times.items()}, "s_all": times,
            "lockstep_over_sequential": med["lockstep"] / med["sequential"],
            "recorded_launches": recs,
            "recorded_launches_per_pass": {k: sum(v.values()) / passes for k, v in recs.items()}}


def main():
    a = sys.argv
    Rs = [int(x) for x in a[1].split(",")] if len(a) > 1 else [4]
    ns = [int(x) for x in a[2].split(",")] if len(a) > 2 else [13]
    mixed = len(a) > 3 and a[3] == "mixed"
    which = a[4] if len(a) > 4 else "anderson"
    reps = int(a[5]) if len(a) > 5 else 15
    if which not in ("anderson", "picard"):
        raise SystemExit("solver: anderson | picard")
    if not torch.cuda.is_available():
        raise SystemExit("fpiter_batch_bench.py measures on the GPU; there is none here")
    w = np.load(os.path.join(ROOT, "tests", "golden", "weights_mixed.npz" if mixed else "weights_dirichlet.npz"))
    sd = {k: torch.from_numpy(w[k]) for k in w.files}
    dev = torch.device("cuda:0")
    net = (pkg("mixed") if mixed else pkg("model_psignn")).ModelPSIGNN(dict(latent_dim=10, n_layers=1))
    net.load_state_dict(sd)
    net = net.to(dev).eval()
    path = os.path.join(ROOT, "profiles", "fpiter_batch_bench.json")
    try:
        book = json.load(open(path))
    except (OSError, ValueError):
        book = {}
    for n in ns:
        for R in Rs:
            out = measure(R, n, mixed, which, reps, dev, net)
            print(json.dumps({k: v for k, v in out.items() if k != "s_all"}), flush=True)
            book[f"{out['solver']}_{out['family']}_R{R}_n{n}"] = out
    with open(path, "w") as fh:
        json.dump(book, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
