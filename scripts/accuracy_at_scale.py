"""How far the decoded u is from the FEM solution on meshes far larger than the training set, and what the classical solve costs.

The shipped dirichlet and mixed checkpoints (tests/golden/weights_*.npz) on hexagon meshes of about 27k, 100k, 270k and 1M nodes.
Ground truth: ``make_hex_problem(..., compute_sol="device")`` (the float64 conjugate-gradient solve on the GPU, tol 1e-12).  Model:
``ModelPSIGNN.eval()`` at the reference's fw_tol 1e-5 / fw_thres 500.  Per size: MSE and relative L2 error of u against sol (the
reference's metric is the MSE), the Broyden ``lowest`` and iteration count; the PCG at its default tol 1e-10: iterations, true
residual, solve time (host clock around the synchronous solve; one warm-up solve, then ``--repeats`` timed ones: median, min, max),
microseconds per iteration, the iteration's algorithmic bytes (ELL values + columns + vectors, each once) and their rate as a
fraction of the HBM peak; and the host's ``spsolve`` time where it finishes within ``--spsolve-limit`` seconds (run in a child
process that never opens the GPU; "not finished" otherwise, "not run" above ``--spsolve-max-nodes``).

    python scripts/accuracy_at_scale.py [--nodes 27000 100000 270000 1000000] [--out profiles/accuracy_at_scale.json]
"""
import argparse, importlib, json, os, subprocess, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12   # bytes/s, MI355X spec


def spsolve_child(n, mixed):
    """Child mode: assemble on the host, time the direct solve alone, print the seconds.  Never touches the GPU."""
    hm = importlib.import_module("psi-gnn_amd.data.hexmesh")
    box = {}
    real = hm._solve

    def timed(A, rhs, compute_sol):
        t0 = time.perf_counter(); out = real(A, rhs, compute_sol); box["s"] = time.perf_counter() - t0
        return out
    hm._solve = timed
    hm.make_hex_problem(n, seed=0, mixed=mixed, compute_sol=True)
    print("SPSOLVE_SECONDS", box["s"], flush=True)


def spsolve_seconds(n, mixed, limit):
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--spsolve-child", str(n), str(int(mixed))],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=limit + 90)   # + assembly
    except subprocess.TimeoutExpired:
        return "not finished"
    for line in r.stdout.splitlines():
        if line.startswith("SPSOLVE_SECONDS"):
            s = float(line.split()[1])
            return s if s <= limit else "not finished"
    return "failed"


def ell_slots(plan):
    """Slots of the solver's 64-row sliced ELL: every slice as deep as its longest free row."""
    a_ptr, flags = plan.export("a_ptr").astype(np.int64), plan.export("node_flags")
    ln = np.where(flags & 1, 0, np.diff(a_ptr))
    ln = np.pad(ln, (0, -len(ln) % 64)).reshape(-1, 64)
    return int(ln.max(1).sum()) * 64, int(ln.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, nargs="+", default=[27_000, 100_000, 270_000, 1_000_000])
    ap.add_argument("--families", nargs="+", default=["dirichlet", "mixed"])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--spsolve-limit", type=float, default=60.0)
    ap.add_argument("--spsolve-max-nodes", type=int, default=300_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "accuracy_at_scale.json"))
    ap.add_argument("--spsolve-child", nargs=2, default=None)
    args = ap.parse_args()
    if args.spsolve_child:
        return spsolve_child(int(args.spsolve_child[0]), bool(int(args.spsolve_child[1])))
    pkg = importlib.import_module("psi-gnn_amd"); eng = importlib.import_module("psi-gnn_amd.engine")
    assert torch.cuda.is_available(), "accuracy_at_scale.py measures on the GPU"
    dev = torch.device("cuda:0")
    rows = []
    for family in args.families:
        mixed = family == "mixed"
        w = np.load(os.path.join(ROOT, "tests", "golden", f"weights_{family}.npz")); sd = {k: torch.from_numpy(w[k]) for k in w.files}
        mod = importlib.import_module("psi-gnn_amd.mixed" if mixed else "psi-gnn_amd.model_psignn")
        net = mod.ModelPSIGNN(dict(latent_dim=10, n_layers=1, fw_tol=1e-5, fw_thres=500)); net.load_state_dict(sd); net = net.to(dev).eval()
        for target in args.nodes:
            n = pkg.data.hex_n_for_nodes(target)
            t0 = time.perf_counter()
            mesh = pkg.data.make_hex_problem(n, seed=0, mixed=mixed, compute_sol="device")
            t_gen = time.perf_counter() - t0
            b = mesh.to(dev)
            # the model
            _, out = net._solve(b)
            u = net.autoencoder.decoder(out["result"]).double()
            sol = b.sol.double()
            row = {"family": family, "n": n, "nodes": mesh.num_nodes, "generate_s": t_gen,
                   "mse": float(torch.mean((u - sol) ** 2)), "rel_l2": float((u - sol).norm() / sol.norm()),
                   "sol_rms": float(sol.pow(2).mean().sqrt()), "broyden_lowest": float(out["lowest"]), "broyden_nstep": int(out["nstep"])}
            # the classical solve, float32 inputs as the model sees them (widened exactly), default tolerance
            plan = eng.plan_for(b)
            cg = eng.PoissonCG(plan, b.a_ij)
            res = cg.solve(b.y)    # warm-up: code objects, allocations of this shape
            times = []
            for _ in range(args.repeats):
                torch.cuda.synchronize(); t0 = time.perf_counter()
                res = cg.solve(b.y)
                times.append(time.perf_counter() - t0)
            cg.close()
            slots, nnz_free = ell_slots(plan)
            bytes_it = 12 * slots + 96 * mesh.num_nodes
            t_med = float(np.median(times))
            us_it = 1e6 * t_med / max(res["n_iter"], 1)
            row.update({"pcg_tol": 1e-10, "pcg_iters": res["n_iter"], "pcg_converged": res["converged"], "pcg_true_rel": res["true_rel"],
                        "pcg_rel": res["rel"], "pcg_solve_s": t_med, "pcg_solve_s_min": float(min(times)), "pcg_solve_s_max": float(max(times)),
                        "pcg_us_per_iter": us_it, "pcg_max_iter_default": eng.default_cg_max_iter(mesh.num_nodes),
                        "ell_slots": slots, "ell_fill": nnz_free / max(slots, 1), "pcg_bytes_per_iter": bytes_it,
                        "pcg_bytes_per_s": bytes_it / (us_it * 1e-6), "pcg_fraction_of_hbm_peak": bytes_it / (us_it * 1e-6) / HBM_PEAK,
                        "pcg_f32_inputs_vs_sol_rel_l2": float((res["result"] - sol).norm() / sol.norm())})
            row["spsolve_s"] = spsolve_seconds(n, mixed, args.spsolve_limit) if mesh.num_nodes <= args.spsolve_max_nodes else "not run"
            print(json.dumps(row), flush=True)
            rows.append(row)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            json.dump({"hbm_peak_bytes_per_s": HBM_PEAK, "rows": rows}, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
