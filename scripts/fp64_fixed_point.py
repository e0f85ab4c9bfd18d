"""Does float64 get below the fp32 floor of the fixed-point solve on large meshes?

The shipped dirichlet and mixed checkpoints (tests/golden/weights_*.npz) on the hexagon meshes of accuracy_at_scale.py (about 27k,
100k, 270k and 1M nodes).  Per mesh two solves from the same start h0 = encoder(x):

* the fp32 device Broyden at the reference's fw_tol 1e-5 / fw_thres 500 (``engine.DeviceBroyden``),
* the float64 device Broyden (``engine.DeviceBroyden64``) at ``--eps64`` 1e-10, threshold ``--threshold64`` 500.

Recorded: ``lowest`` and the step counts of both; the relative L2 distance between the two results and between their decoded u (both
decoded in float64); the float64 solve's wall time per iteration (host clock around the synchronous solve) and its algorithmic bytes
per iteration over the HBM peak of 8 TB/s.  The byte count is what the solve's launch sites state (every operand once): with k stored
pairs an iteration streams (4 k + 26) M doubles through the solver's kernels (M = 10 N), plus f; the file holds the mean over the
iterations actually run.

    python scripts/fp64_fixed_point.py [--nodes 27000 100000 270000 1000000] [--out profiles/fp64_fixed_point.json]
"""
import argparse, importlib, json, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12   # bytes/s, MI355X spec


def solver_bytes(n_iter, threshold, M, Ep, N, P):
    """Algorithmic bytes of a float64 solve of n_iter steps: per step the vector kernels (step 4 M, residual 5 M, keep <= 2 M) and,
    while a pair is still stored (step < threshold), sweep 1 (2 k + 3) M, sweep 2 (2 k + 6) M and the apply 4 M doubles; one f per
    step: both edge lists once (neighbour id, three attributes, the neighbour's row) and per node its rows, prb and flags."""
    f_bytes = 2 * Ep * (4 + 24 + 80) + N * (160 + 8 * P + 17)
    total = 0
    for it in range(1, n_iter + 1):
        k = it - 1
        total += 8 * M * (4 + 5 + 2) + f_bytes
        if it < threshold:
            total += 8 * M * ((2 * k + 3 if k else 0) + (2 * k + 6) + 4)
    return total


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, nargs="+", default=[27_000, 100_000, 270_000, 1_000_000])
    ap.add_argument("--families", nargs="+", default=["dirichlet", "mixed"])
    ap.add_argument("--eps64", type=float, default=1e-10)
    ap.add_argument("--threshold64", type=int, default=500)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fp64_fixed_point.json"))
    args = ap.parse_args()
    pkg = importlib.import_module("psi-gnn_amd"); eng = importlib.import_module("psi-gnn_amd.engine")
    assert torch.cuda.is_available(), "fp64_fixed_point.py measures on the GPU"
    dev = torch.device("cuda:0")
    rows = []
    for family in args.families:
        mixed = family == "mixed"
        w = np.load(os.path.join(ROOT, "tests", "golden", f"weights_{family}.npz")); sd = {k: torch.from_numpy(w[k]) for k in w.files}
        ae = lambda which: [sd[f"autoencoder.{which}.mlp.mlp.{i}.{p}"] for i, p in ((0, "weight"), (0, "bias"), (2, "weight"), (2, "bias"))]
        for target in args.nodes:
            n = pkg.data.hex_n_for_nodes(target)
            b = pkg.data.make_hex_problem(n, seed=0, mixed=mixed, compute_sol=False).to(dev)
            plan = eng.plan_for(b)
            nrm = getattr(b, "unit_normal_vector", None)
            h0_64 = eng.mlp2_64(b.x, *ae("encoder"))
            # fp32, as the model runs it, from the same start rounded to float32
            fm32 = eng.FixedPointMap(plan, eng.PackedWeights(sd, dev), h0_64, b.prb_data, nrm)
            sv32 = eng.DeviceBroyden(plan, threshold=500)
            o32 = sv32.solve(fm32, 1e-5)
            sv32.close()
            fm64 = eng.FixedPointMap64(plan, eng.PackedWeights64(sd), h0_64, b.prb_data, b.edge_attr, nrm)
            sv64 = eng.DeviceBroyden64(fm64, args.threshold64)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            o64 = sv64.solve(h0_64, args.eps64)
            t64 = time.perf_counter() - t0
            nbytes = sv64.nbytes
            sv64.close(); fm64.close()
            u32 = eng.mlp2_64(o32["result"], *ae("decoder"))
            u64 = eng.mlp2_64(o64["result"], *ae("decoder"))
            M = 10 * plan.N
            alg = solver_bytes(o64["n_iter"], args.threshold64, M, plan.Ep, plan.N, 3 if mixed else 2)
            us_it = 1e6 * t64 / max(o64["n_iter"], 1)
            row = {"family": family, "n": n, "nodes": plan.N, "fp32_lowest": float(o32["lowest"]), "fp32_nstep": int(o32["nstep"]),
                   "fp32_n_iter": int(o32["n_iter"]), "fp64_eps": args.eps64, "fp64_threshold": args.threshold64,
                   "fp64_lowest": float(o64["lowest"]), "fp64_nstep": int(o64["nstep"]), "fp64_n_iter": int(o64["n_iter"]),
                   "fp64_stop_reason": int(o64["stop_reason"]), "h_rel_l2_fp32_vs_fp64": rel_l2(o32["result"], o64["result"]),
                   "u_rel_l2_fp32_vs_fp64": rel_l2(u32, u64), "fp64_solve_s": t64, "fp64_us_per_iter": us_it,
                   "fp64_solver_bytes": nbytes, "fp64_alg_bytes_per_iter": alg / max(o64["n_iter"], 1),
                   "fp64_fraction_of_hbm_peak": alg / t64 / HBM_PEAK}
            print(json.dumps(row), flush=True)
            rows.append(row)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            json.dump({"hbm_peak_bytes_per_s": HBM_PEAK, "rows": rows}, open(args.out, "w"), indent=1)
            del fm32, sv32, fm64, sv64, o32, o64, b, plan
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
