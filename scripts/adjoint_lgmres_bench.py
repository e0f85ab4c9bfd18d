"""Does the stall of the fp32 GMRES adjoint solve at scale (``bw_solver = "gmres"``: "stagnation" at the first cycle that does not halve
``rel``) move when the halving rule is lifted, and when the restarts keep a correction (LGMRES)?  The float64 solver's answer is
profiles/fp64_lgmres.json; this is the same question for the solver training runs.

The inputs of fp64_lgmres.py: the shipped dirichlet and mixed checkpoints on the hexagon meshes of 27 361, 101 017, 270 901 and
1 000 519 nodes, the state H = the fp32 device Broyden result at fw_tol 1e-5 / fw_thres 500 from h0 = encoder(x), grad = randn
(seed 3), the system y = J_f(H)^T y + grad on the stored linearisation at H (mixed: Neumann rows stored), the route training takes
with ``bw_linearize``.  Per mesh, on one ``DeviceGmresAug(m = 50, augment = 1)`` in one process, eps 1e-8 (the launch ``bw_tol``),
budgets 500 and 2 000:

* (augment 0, stall 0.5): today's solve, the baseline (the kernels and the bits of ``DeviceGmres``);
* (0, 1.0), (1, 1.0).

Recorded per solve: products, cycles, ``n_aug``, stop reason, ``lowest`` and the wall time of the call (one run, after one two-product
solve that makes the workspace), and beside it the float64 run of profiles/fp64_lgmres.json with the same (augment, stall) on the
same mesh (eps 1e-11, budget 2 000), where that file has one.

Every mesh runs in a child process of its own under a time limit; the meshes are chained, and after a child that failed or ran out
of time nothing more is started.  Nothing is gated.

    python scripts/adjoint_lgmres_bench.py [--nodes 27000 100000 270000 1000000] [--families dirichlet mixed] [--out profiles/adjoint_lgmres.json]
"""
import argparse, importlib, json, os, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
RUNS = [(0, 0.5), (0, 1.0), (1, 1.0)]
BUDGETS = [500, 2000]


def one_mesh(args):
    import numpy as np, torch
    pkg = importlib.import_module("psi-gnn_amd"); eng = importlib.import_module("psi-gnn_amd.engine")
    assert torch.cuda.is_available(), "adjoint_lgmres_bench.py measures on the GPU"
    dev = torch.device("cuda:0")
    family, target = args.one[0], int(args.one[1])
    mixed = family == "mixed"
    w = np.load(os.path.join(ROOT, "tests", "golden", f"weights_{family}.npz")); sd = {k: torch.from_numpy(w[k]) for k in w.files}
    enc = [sd[f"autoencoder.encoder.mlp.mlp.{i}.{p}"] for i, p in ((0, "weight"), (0, "bias"), (2, "weight"), (2, "bias"))]
    n = pkg.data.hex_n_for_nodes(target)
    b = pkg.data.make_hex_problem(n, seed=0, mixed=mixed, compute_sol=False).to(dev)
    plan = eng.plan_for(b)
    nrm = getattr(b, "unit_normal_vector", None)
    h0 = eng.mlp2_64(b.x, *enc)
    fmap = eng.FixedPointMap(plan, eng.PackedWeights(sd, dev), h0, b.prb_data, nrm)
    sv = eng.DeviceBroyden(plan, threshold=500)
    fw = sv.solve(fmap, 1e-5)
    H = fw["result"]
    sv.close()
    del sv
    grad = torch.randn(H.shape, generator=torch.Generator().manual_seed(3)).to(dev)
    lin = fmap.linearize_p(fmap.to_plan(H), neumann="stored" if mixed else "direct")
    row = {"family": family, "n": n, "nodes": plan.N, "forward_lowest": float(fw["lowest"]), "runs": []}
    gm = eng.DeviceGmresAug(plan.N * eng.D, dev, args.m, augment=max(a for a, _ in RUNS))
    gm.solve_adjoint(fmap, H, grad, args.eps, 2, lin=lin)   # makes the workspace and the traces
    row["gmres_bytes"] = int(gm.nbytes)
    for budget in BUDGETS:
        for augment, stall in RUNS:
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            g = gm.solve_adjoint(fmap, H, grad, args.eps, budget, lin=lin, augment=augment, stall=stall)
            torch.cuda.synchronize(dev)
            ms = 1e3 * (time.perf_counter() - t0)
            row["runs"].append({"augment": augment, "stall": stall, "budget": budget, "products": int(g["nstep"]), "cycles": int(g["n_cycles"]),
                                "n_aug": int(g["n_aug"]), "stop": str(g["stop"]), "lowest": float(g["lowest"]), "n_reorth": int(g["n_reorth"]),
                                "wall_ms": ms, "rel_trace": g["rel_trace"]})
            print(json.dumps({k: v for k, v in row["runs"][-1].items() if k != "rel_trace"} | {"nodes": plan.N, "family": family}), flush=True)
            del g
    gm.close()
    lin.close()
    json.dump(row, open(args.out, "w"))


def float64_runs(path):
    """{(family, nodes, augment, stall): the float64 run's products / stop / lowest} of profiles/fp64_lgmres.json."""
    if not os.path.exists(path):
        return {}
    out = {}
    for row in json.load(open(path)).get("rows", []):
        for r in row["runs"]:
            out[(row["family"], row["nodes"], r["augment"], r["stall"])] = {k: r[k] for k in ("products", "cycles", "n_aug", "stop", "lowest")}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, nargs="+", default=[27_000, 100_000, 270_000, 1_000_000])
    ap.add_argument("--families", nargs="+", default=["dirichlet", "mixed"])
    ap.add_argument("--m", type=int, default=50)
    ap.add_argument("--eps", type=float, default=1e-8)
    ap.add_argument("--mesh-timeout", type=int, default=300, help="seconds one mesh's child process may take")
    ap.add_argument("--float64", default=os.path.join(ROOT, "profiles", "fp64_lgmres.json"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adjoint_lgmres.json"))
    ap.add_argument("--one", nargs=2, metavar=("FAMILY", "NODES"), help="(internal) one mesh in this process, the row written to --out")
    args = ap.parse_args()
    if args.one:
        return one_mesh(args)
    f64 = float64_runs(args.float64)
    doc = {"settings": {"eps": args.eps, "m": args.m, "budgets": BUDGETS, "runs": RUNS, "route": "stored linearisation (lin.vjp_p)",
                        "float64": "profiles/fp64_lgmres.json: eps 1e-11, budget 2000, m 50"}, "rows": []}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for family in args.families:
        for target in args.nodes:
            with tempfile.TemporaryDirectory() as tmp:
                part = os.path.join(tmp, "row.json")
                cmd = [sys.executable, os.path.abspath(__file__), "--one", family, str(target), "--m", str(args.m), "--eps", str(args.eps),
                       "--out", part]
                try:
                    rc = subprocess.run(cmd, timeout=args.mesh_timeout).returncode
                except subprocess.TimeoutExpired:
                    rc = 124
                if rc != 0:   # a fault, an abort or a hang: nothing more is started
                    doc["stopped"] = f"{family} {target}: exit status {rc}; the remaining meshes were not run"
                    json.dump(doc, open(args.out, "w"), indent=1)
                    print(doc["stopped"], flush=True)
                    return rc
                row = json.load(open(part))
            for r in row["runs"]:
                r["float64"] = f64.get((row["family"], row["nodes"], r["augment"], r["stall"]))
            doc["rows"].append(row)
            json.dump(doc, open(args.out, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
