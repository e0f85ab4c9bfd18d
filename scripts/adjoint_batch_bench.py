"""The adjoint solve alone: ``engine.broyden_solve_adjoint_batch`` over R replicas against R single
``DeviceBroyden.solve_adjoint(lin=)`` calls on the SAME solver objects and linearisations (so both do the same iterations, bit for
bit), at the reference's training shape: every replica a union batch of hexagon meshes, H* from the forward batched solve.

    python3 scripts/adjoint_batch_bench.py [replicas=4] [graphs_per_batch=50] [hex_n=13] [repeats=5] [family=dirichlet|mixed]

Prints one JSON line: median seconds of either route (alternated), lockstep iterations per second, launches per iteration of either
route from the library's per-kernel records."""
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


def main():
    a = sys.argv
    R = int(a[1]) if len(a) > 1 else 4
    B = int(a[2]) if len(a) > 2 else 50
    n = int(a[3]) if len(a) > 3 else 13
    reps = int(a[4]) if len(a) > 4 else 5
    mixed = len(a) > 5 and a[5] == "mixed"
    fw_tol, bw_tol, thr = 1e-5, 1e-8, 500
    data, eng, nat = pkg("data"), pkg("engine"), pkg("_native")
    w = np.load(os.path.join(ROOT, "tests", "golden", "weights_mixed.npz" if mixed else "weights_dirichlet.npz"))
    sd = {k: torch.from_numpy(w[k]) for k in w.files}
    dev = torch.device("cuda:0")
    net = (pkg("mixed") if mixed else pkg("model_psignn")).ModelPSIGNN(dict(latent_dim=10, n_layers=1, fw_tol=fw_tol, fw_thres=thr))
    net.load_state_dict(sd)
    net = net.to(dev).eval()
    batches = [data.collate([data.make_hex_problem(n, seed=r * B + s, phase=0.37 * (r * B + s), mixed=mixed, compute_sol=False)
                             for s in range(B)]).to(dev) for r in range(R)]
    with torch.no_grad():
        fmaps = [net.deqdss.f.bind(net.autoencoder.encoder(b.x), b) for b in batches]
    total = sum(f.plan.N for f in fmaps) * 10
    fw = [eng.DeviceBroyden(plan=f.plan, threshold=thr, shard_elems=total) for f in fmaps]
    H = [o["result"] for o in eng.broyden_solve_batch(fw, fmaps, fw_tol)]
    for sv in fw:
        sv.close()
    lins = [f.linearize_p(f.to_plan(h), neumann="stored" if mixed else None) for f, h in zip(fmaps, H)]
    grads = [torch.randn(h.shape, generator=torch.Generator().manual_seed(7 + i)).to(dev) for i, h in enumerate(H)]
    solvers = [eng.DeviceBroyden(plan=f.plan, threshold=thr, shard_elems=total) for f in fmaps]
    assert eng.adjoint_batchable(solvers, lins)
    routes = {"lockstep": lambda: eng.broyden_solve_adjoint_batch(solvers, lins, grads, bw_tol),
              "single": lambda: [sv.solve_adjoint(f, h, g, bw_tol, lin=l) for sv, f, h, g, l in zip(solvers, fmaps, H, grads, lins)]}
    outs = {k: f() for k, f in routes.items()}   # warm-up
    same = all(x["n_iter"] == y["n_iter"] and torch.equal(x["result"], y["result"]) for x, y in zip(outs["lockstep"], outs["single"]))
    torch.cuda.synchronize()
    times = {k: [] for k in routes}
    for _ in range(reps):
        for k, f in routes.items():
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t0)
    nat.prof_enable(True)
    launches = {}
    for k, f in routes.items():
        nat.prof_collect()
        f()
        torch.cuda.synchronize()
        launches[k] = sum(v[0] for v in nat.prof_collect().values())
    nat.prof_enable(False)
    its = [o["n_iter"] for o in outs["lockstep"]]
    med = {k: statistics.median(v) for k, v in times.items()}
    print(json.dumps({
        "workload": f"adjoint solve ({'mixed' if mixed else 'dirichlet'} family), {R} replicas, each a union batch of {B} hexagon meshes "
                    f"(n={n}): {fmaps[0].plan.N} nodes per replica; bw_tol {bw_tol}, threshold {thr}",
        "replicas": R, "n_iter": its, "bit_identical": same, "s_median": med, "s_all": times,
        "lockstep_over_single": med["lockstep"] / med["single"],
        "lockstep_iterations_per_s": max(its) / med["lockstep"], "single_iterations_per_s": sum(its) / med["single"],
        "replica_iterations_per_s_lockstep": sum(its) / med["lockstep"],
        "launches_per_lockstep_iteration": launches["lockstep"] / max(its),
        "launches_per_single_iteration": launches["single"] / sum(its)}))


if __name__ == "__main__":
    main()
