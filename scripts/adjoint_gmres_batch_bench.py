"""The GMRES adjoint solve alone: ``engine.gmres_solve_adjoint_batch`` over R replicas against R single
``DeviceGmres.solve_adjoint(lin=)`` calls on the SAME handles and linearisations (so both do the same cycles and products, bit for
bit), at the reference's training shape: every replica a union batch of hexagon meshes, H* from the forward batched solve.

    python3 scripts/adjoint_gmres_batch_bench.py [replicas=4] [graphs_per_batch=50] [hex_n=13] [repeats=5] [family=dirichlet|mixed]

bw 1e-8 / 500, restart length 50.  Prints one JSON line and stores it in profiles/adjoint_gmres_batch_bench.json (one entry per
family and replica count): median seconds of either route (alternated), the bit-identity check, and from the library's per-kernel
records the launches of either route and the launches per lockstep Arnoldi step."""
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
FIELDS = ("nstep", "n_cycles", "stop", "n_reorth", "lowest", "lowest_abs", "rel_trace", "abs_trace")
STEP_KERNELS = ("k_vjp_lin_batch", "k_gm_dots_batch", "k_gm_reduce_batch", "k_gm_axpy_batch", "k_gm_decide_batch", "k_gm_finish_batch",
                "k_gm_scale_batch")


def main():
    a = sys.argv
    R = int(a[1]) if len(a) > 1 else 4
    B = int(a[2]) if len(a) > 2 else 50
    n = int(a[3]) if len(a) > 3 else 13
    reps = int(a[4]) if len(a) > 4 else 5
    mixed = len(a) > 5 and a[5] == "mixed"
    fw_tol, bw_tol, thr, m = 1e-5, 1e-8, 500, 50
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
    solvers = [eng.DeviceGmres(f.plan.N * 10, dev, m, shard_elems=total) for f in fmaps]
    assert eng.gmres_adjoint_batchable(solvers, lins)
    routes = {"lockstep": lambda: eng.gmres_solve_adjoint_batch(solvers, lins, grads, bw_tol, thr),
              "single": lambda: [sv.solve_adjoint(f, h, g, bw_tol, thr, lin=l) for sv, f, h, g, l in zip(solvers, fmaps, H, grads, lins)]}
    outs = {k: f() for k, f in routes.items()}   # warm-up
    same = all(all(x[q] == y[q] for q in FIELDS) and torch.equal(x["result"], y["result"]) for x, y in zip(outs["lockstep"], outs["single"]))
    torch.cuda.synchronize()
    times = {k: [] for k in routes}
    for _ in range(reps):
        for k, f in routes.items():
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t0)
    nat.prof_enable(True)
    launches, recs = {}, {}
    for k, f in routes.items():
        nat.prof_collect()
        f()
        torch.cuda.synchronize()
        recs[k] = nat.prof_collect()
        launches[k] = sum(v[0] for v in recs[k].values())
    nat.prof_enable(False)
    lock = recs["lockstep"]
    arnoldi_steps = lock["k_gm_finish_batch"][0]
    nstep = [o["nstep"] for o in outs["lockstep"]]
    med = {k: statistics.median(v) for k, v in times.items()}
    out = {
        "workload": f"GMRES({m}) adjoint solve ({'mixed' if mixed else 'dirichlet'} family), {R} replicas, each a union batch of {B} "
                    f"hexagon meshes (n={n}): {fmaps[0].plan.N} nodes per replica; bw_tol {bw_tol}, budget {thr}",
        "family": "mixed" if mixed else "dirichlet", "replicas": R, "products": nstep, "cycles": [o["n_cycles"] for o in outs["lockstep"]],
        "stops": [o["stop"] for o in outs["lockstep"]], "bit_identical": same, "s_median": med, "s_all": times,
        "lockstep_over_single": med["lockstep"] / med["single"],
        "launches": launches, "lockstep_arnoldi_steps": arnoldi_steps,
        # (per lockstep cycle one scale launch belongs to the cycle's start, and after the first cycle one product to its residual)
        "launches_per_lockstep_arnoldi_step": (sum(lock[q][0] for q in STEP_KERNELS if q in lock) - 2 * lock["k_ag_check_batch"][0] + 1)
                                              / max(arnoldi_steps, 1),
        "launches_per_single_product": launches["single"] / max(sum(nstep), 1)}
    print(json.dumps(out))
    path = os.path.join(ROOT, "profiles", "adjoint_gmres_batch_bench.json")
    try:
        book = json.load(open(path))
    except (OSError, ValueError):
        book = {}
    book[f"{out['family']}_R{R}_B{B}_n{n}"] = out
    with open(path, "w") as fh:
        json.dump(book, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
