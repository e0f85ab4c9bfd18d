"""Does the at-scale stall of the float64 adjoint GMRES ("stagnation after the second cycle" at lowest
3.5e-3 - 5.1e-3) move when the halving rule is lifted, and when the restarts keep corrections (LGMRES)?

The inputs of fp64_adjoint.py: the shipped dirichlet and mixed checkpoints on the hexagon meshes of 27 361, 101 017, 270 901 and
1 000 519 nodes, the state H = the fp32 device Broyden result at fw_tol 1e-5 / fw_thres 500 from h0 = encoder(x), grad = randn
(seed 3), the system y = J_f(H)^T y + grad.  Per mesh, on one ``DeviceGmres64Aug(m = 50, augment = 3)`` in one process, eps 1e-11,
budget 2000:

* (stall 0.5, augment 0): today's solve, the baseline (the kernels and the bits of ``DeviceGmres64``);
* (1.0, 0), (1.0, 1), (1.0, 2), (1.0, 3).

Recorded per run: products, cycles, ``n_aug``, stop reason, ``lowest``, the ``rel_trace``, microseconds per Arnoldi step and per
augmentation step (the ``k_gm64_*`` kernels of a step plus ``k_lg64_shift``, the product aside) from the library's launch records
with their algorithmic bytes as a fraction of the HBM peak (8 TB/s), and ``nbytes``.  The runs poll after every step
(``poll_every = 1``, which changes neither bits nor counts), so that every recorded launch did work.  Then one ``DeviceNewton64Aug(m
= 50, augment = 2)`` solve from h0 with ``lin_stall = 1.0`` against ``DeviceNewton64(m = 50)``, eps 1e-11, threshold 50.

Every mesh runs in a child process of its own under a time limit; the meshes are chained, and after a child that failed or ran out
of time nothing more is started.  Nothing is gated.

    python scripts/fp64_lgmres.py [--nodes 27000 100000 270000 1000000] [--families dirichlet mixed] [--out profiles/fp64_lgmres.json]
"""
import argparse, importlib, json, os, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK_GBS = 8000.0
RUNS = [(0.5, 0), (1.0, 0), (1.0, 1), (1.0, 2), (1.0, 3)]
STEP = ("k_gm64_dots", "k_gm64_reduce", "k_gm64_axpy", "k_gm64_decide", "k_gm64_finish", "k_gm64_scale", "k_lg64_shift")


def step_times(log):
    """(Arnoldi steps, ms, bytes), (augmentation steps, ms, bytes) of one solve's launch log: a step is what lies between a product
    and the ``k_gm64_scale`` that follows ``k_gm64_finish``; it is an augmentation step when ``k_lg64_shift`` is in it."""
    acc = {False: [0, 0.0, 0], True: [0, 0.0, 0]}
    ms = by = 0.0
    aug = in_step = False
    prev = None
    for name, t, b in log:
        if name.startswith("k_f64_"):   # a product: a step (or a cycle's residual) begins
            ms, by, aug, in_step = 0.0, 0, False, True
        elif in_step and name in STEP:
            ms, by = ms + t, by + b
            aug |= name == "k_lg64_shift"
            if name == "k_gm64_scale" and prev == "k_gm64_finish":
                a = acc[aug]
                a[0], a[1], a[2] = a[0] + 1, a[1] + ms, a[2] + by
                in_step = False
        else:
            in_step = False
        prev = name
    return acc[False], acc[True]


def one_mesh(args):
    import numpy as np, torch
    pkg = importlib.import_module("psi-gnn_amd"); eng = importlib.import_module("psi-gnn_amd.engine")
    nat = importlib.import_module("psi-gnn_amd._native")
    assert torch.cuda.is_available(), "fp64_lgmres.py measures on the GPU"
    dev = torch.device("cuda:0")
    family, target = args.one[0], int(args.one[1])
    mixed = family == "mixed"
    w = np.load(os.path.join(ROOT, "tests", "golden", f"weights_{family}.npz")); sd = {k: torch.from_numpy(w[k]) for k in w.files}
    enc = [sd[f"autoencoder.encoder.mlp.mlp.{i}.{p}"] for i, p in ((0, "weight"), (0, "bias"), (2, "weight"), (2, "bias"))]
    n = pkg.data.hex_n_for_nodes(target)
    b = pkg.data.make_hex_problem(n, seed=0, mixed=mixed, compute_sol=False).to(dev)
    plan = eng.plan_for(b)
    nrm = getattr(b, "unit_normal_vector", None)
    h0_64 = eng.mlp2_64(b.x, *enc)
    fm32 = eng.FixedPointMap(plan, eng.PackedWeights(sd, dev), h0_64, b.prb_data, nrm)
    fm64 = eng.FixedPointMap64(plan, eng.PackedWeights64(sd), h0_64, b.prb_data, b.edge_attr, nrm)
    sv = eng.DeviceBroyden(plan, threshold=500)
    fw = sv.solve(fm32, 1e-5)
    H = fw["result"]
    sv.close()
    del sv, fm32
    grad = torch.randn(H.shape, generator=torch.Generator().manual_seed(3)).to(dev)
    row = {"family": family, "n": n, "nodes": plan.N, "forward_lowest": float(fw["lowest"]), "runs": [], "newton": []}
    gm = eng.DeviceGmres64Aug(fm64, args.m, max(a for _, a in RUNS))
    row["gmres64_bytes"] = int(gm.nbytes)
    for stall, augment in RUNS:
        nat.prof_enable(True); nat.prof_collect()
        g = gm.solve_adjoint(H, grad, args.eps, args.max_products, poll_every=1, augment=augment, stall=stall)
        nat.prof_collect(); nat.prof_enable(False)
        (ns, ms, by), (na, msa, bya) = step_times(nat.prof_launch_log())
        frac = lambda bb, mm: (bb / (mm * 1e-3) / 1e9 / HBM_PEAK_GBS) if mm else None
        row["runs"].append({"stall": stall, "augment": augment, "products": int(g["nstep"]), "cycles": int(g["n_cycles"]),
                            "n_aug": int(g["n_aug"]), "stop": str(g["stop"]), "lowest": float(g["lowest"]), "n_reorth": int(g["n_reorth"]),
                            "rel_trace": g["rel_trace"], "arnoldi_steps_timed": ns, "arnoldi_step_us": 1e3 * ms / ns if ns else None,
                            "arnoldi_step_frac_of_hbm_peak": frac(by, ms), "augmentation_steps_timed": na,
                            "augmentation_step_us": 1e3 * msa / na if na else None,
                            "augmentation_step_frac_of_hbm_peak": frac(bya, msa)})
        print(json.dumps({k: v for k, v in row["runs"][-1].items() if k != "rel_trace"} | {"nodes": plan.N, "family": family}), flush=True)
        del g
    gm.close()
    del gm
    torch.cuda.empty_cache()
    for name, make, kw in (("default", lambda: eng.DeviceNewton64(fm64, args.m), {}),
                           ("augment 2, lin_stall 1.0", lambda: eng.DeviceNewton64Aug(fm64, args.m, 2), {"lin_stall": 1.0})):
        nt = make()
        o = nt.solve(h0_64, eps=args.eps, threshold=50, **kw)
        row["newton"].append({"solver": name, "stop": o["stop_reason"], "n_iter": int(o["n_iter"]), "accepted": int(sum(o["accepted"])),
                              "products": int(o["n_products"]), "lowest": float(o["lowest"]), "krylov": list(o["krylov"]),
                              "lin_stop": list(o["lin_stop"]), "bytes": int(nt.nbytes)})
        print(json.dumps({k: v for k, v in row["newton"][-1].items() if k not in ("krylov", "lin_stop")} | {"nodes": plan.N}), flush=True)
        nt.close()
        del nt, o
        torch.cuda.empty_cache()
    fm64.close()
    json.dump(row, open(args.out, "w"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, nargs="+", default=[27_000, 100_000, 270_000, 1_000_000])
    ap.add_argument("--families", nargs="+", default=["dirichlet", "mixed"])
    ap.add_argument("--m", type=int, default=50)
    ap.add_argument("--max-products", type=int, default=2000)
    ap.add_argument("--eps", type=float, default=1e-11)
    ap.add_argument("--mesh-timeout", type=int, default=420, help="seconds one mesh's child process may take")
    ap.add_argument("--resource-usage", default=os.path.join(ROOT, "profiles", "fp64_lgmres_resource_usage.txt"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fp64_lgmres.json"))
    ap.add_argument("--one", nargs=2, metavar=("FAMILY", "NODES"), help="(internal) one mesh in this process, the row written to --out")
    args = ap.parse_args()
    if args.one:
        return one_mesh(args)
    from fp64_derivatives import resource_usage
    doc = {"settings": {"eps": args.eps, "m": args.m, "max_products": args.max_products, "runs": RUNS, "poll_every": 1,
                        "newton": "eps 1e-11, threshold 50, eta 1e-2, 200 products per linear solve", "hbm_peak_GBps": HBM_PEAK_GBS},
           "kernels": resource_usage(args.resource_usage) if os.path.exists(args.resource_usage) else None, "rows": []}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for family in args.families:
        for target in args.nodes:
            with tempfile.TemporaryDirectory() as tmp:
                part = os.path.join(tmp, "row.json")
                cmd = [sys.executable, os.path.abspath(__file__), "--one", family, str(target), "--m", str(args.m), "--max-products",
                       str(args.max_products), "--eps", str(args.eps), "--out", part]
                try:
                    rc = subprocess.run(cmd, timeout=args.mesh_timeout).returncode
                except subprocess.TimeoutExpired:
                    rc = 124
                if rc != 0:   # a fault, an abort or a hang: nothing more is started
                    doc["stopped"] = f"{family} {target}: exit status {rc}; the remaining meshes were not run"
                    json.dump(doc, open(args.out, "w"), indent=1)
                    print(doc["stopped"], flush=True)
                    return rc
                doc["rows"].append(json.load(open(part)))
            json.dump(doc, open(args.out, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
