"""Does the float64 Newton-Krylov solve with a pseudo-transient shift get below the 1e-4 floor at which Broyden stalls on large meshes?

The shipped dirichlet and mixed checkpoints (tests/golden/weights_*.npz) on the hexagon meshes of fp64_fixed_point.py (27 361,
101 017, 270 901 and 1 000 519 nodes).  Per mesh ``engine.DeviceNewton64`` (m 50, eps 1e-11, threshold 50, eta 1e-2, 200 products per
step, growth 2, reject_floor 1/16, sigma_off 1e-8, max_rejects 8 -- the defaults, which are starting values from CPU runs and are not
tuned on a GPU) is run four times: from h0 = encoder(x) and from the result of the fp32 device Broyden (fw_tol 1e-5 / fw_thres 500),
with sigma0 = 1 and sigma0 = 0.

Recorded per run: ``lowest`` and the stop reason, accepted and rejected steps, products, evaluations of f, the sigma trace, the rel
trace, the products and the linear solve's stop reason per attempted step, the wall time of the solve (host clock around the
synchronous call) and from it the time per outer step; next to it ``lowest`` of the float64 Broyden on the same mesh from
profiles/fp64_fixed_point.json.  Per mesh, one more run (from h0, sigma0 = 1, five attempted steps, the host polling after every
Arnoldi step so that every launch runs) under the library's launch records gives the time per product (``k_f64_jvp_layer``) and per
Arnoldi step (the ``k_gm64_*`` launches of a step, without the product).

    python scripts/fp64_newton_krylov.py [--nodes 27000 100000 270000 1000000] [--families dirichlet mixed]
                                         [--out profiles/fp64_newton_krylov.json]
"""
import argparse, importlib, json, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)


def broyden64_lowest(family, nodes):
    """``fp64_lowest`` of the float64 Broyden solve of the same mesh, as profiles/fp64_fixed_point.json holds it (None: not there)."""
    try:
        rows = json.load(open(os.path.join(ROOT, "profiles", "fp64_fixed_point.json")))["rows"]
    except OSError:
        return None
    hit = [r for r in rows if r["family"] == family and r["nodes"] == nodes]
    return float(hit[0]["fp64_lowest"]) if hit else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, nargs="+", default=[27_000, 100_000, 270_000, 1_000_000])
    ap.add_argument("--families", nargs="+", default=["dirichlet", "mixed"])
    ap.add_argument("--m", type=int, default=50)
    ap.add_argument("--eps", type=float, default=1e-11)
    ap.add_argument("--threshold", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fp64_newton_krylov.json"))
    args = ap.parse_args()
    pkg = importlib.import_module("psi-gnn_amd"); eng = importlib.import_module("psi-gnn_amd.engine")
    nat = importlib.import_module("psi-gnn_amd._native")
    assert torch.cuda.is_available(), "fp64_newton_krylov.py measures on the GPU"
    dev = torch.device("cuda:0")
    doc = {"settings": {"m": args.m, "eps": args.eps, "threshold": args.threshold, "eta": 1e-2, "max_products": 200, "growth": 2.0,
                        "reject_floor": 0.0625, "sigma_off": 1e-8, "max_rejects": 8, "fp32_start": "DeviceBroyden 1e-5 / 500",
                        "defaults": "starting values from float64 CPU runs on the stored fixtures, not tuned on a GPU"}, "rows": []}
    if os.path.exists(args.out):   # a run per family may add to the file of the other
        old = json.load(open(args.out))
        doc["rows"] = [r for r in old.get("rows", []) if r["family"] not in args.families]
    for family in args.families:
        mixed = family == "mixed"
        w = np.load(os.path.join(ROOT, "tests", "golden", f"weights_{family}.npz")); sd = {k: torch.from_numpy(w[k]) for k in w.files}
        enc = [sd[f"autoencoder.encoder.mlp.mlp.{i}.{p}"] for i, p in ((0, "weight"), (0, "bias"), (2, "weight"), (2, "bias"))]
        for target in args.nodes:
            n = pkg.data.hex_n_for_nodes(target)
            b = pkg.data.make_hex_problem(n, seed=0, mixed=mixed, compute_sol=False).to(dev)
            plan = eng.plan_for(b)
            nrm = getattr(b, "unit_normal_vector", None)
            h0_64 = eng.mlp2_64(b.x, *enc)
            fm32 = eng.FixedPointMap(plan, eng.PackedWeights(sd, dev), h0_64, b.prb_data, nrm)
            sv32 = eng.DeviceBroyden(plan, threshold=500)
            o32 = sv32.solve(fm32, 1e-5)
            sv32.close()
            h32 = o32["result"].double()
            fm64 = eng.FixedPointMap64(plan, eng.PackedWeights64(sd), h0_64, b.prb_data, b.edge_attr, nrm)
            nt = eng.DeviceNewton64(fm64, args.m)
            row = {"family": family, "n": n, "nodes": plan.N, "fp32_broyden_lowest": float(o32["lowest"]),
                   "fp64_broyden_lowest": broyden64_lowest(family, plan.N), "newton64_bytes": int(nt.nbytes), "runs": []}
            for start, x0 in (("h0", h0_64), ("fp32 result", h32)):
                for sigma0 in (1.0, 0.0):
                    torch.cuda.synchronize(); t0 = time.perf_counter()
                    o = nt.solve(x0, eps=args.eps, threshold=args.threshold, sigma0=sigma0)
                    dt = time.perf_counter() - t0
                    acc = sum(o["accepted"])
                    run = {"start": start, "sigma0": sigma0, "lowest": float(o["lowest"]), "stop_reason": o["stop_reason"],
                           "nstep": int(o["nstep"]), "n_iter": int(o["n_iter"]), "accepted": acc, "rejected": int(o["n_iter"]) - acc,
                           "n_products": int(o["n_products"]), "n_feval": int(o["n_feval"]), "sigma_trace": o["sigma_trace"],
                           "rel_trace": o["rel_trace"], "krylov": o["krylov"], "lin_stop": o["lin_stop"], "solve_s": dt,
                           "outer_step_ms": 1e3 * dt / max(o["n_iter"], 1), "below_1e-4": bool(o["lowest"] < 1e-4)}
                    print(json.dumps({k: v for k, v in run.items() if not isinstance(v, list)} | {"family": family, "nodes": plan.N}),
                          flush=True)
                    row["runs"].append(run)
            # kernel times of a short run under the launch records
            nat.prof_enable(True); nat.prof_collect()
            o = nt.solve(h0_64, eps=args.eps, threshold=5, poll_every=1)   # polled after every step: what is launched runs
            rec = nat.prof_collect(with_bytes=True); nat.prof_enable(False)
            prod_calls = sum(c for k, (c, _, _) in rec.items() if k == "k_f64_jvp_layer")
            prod_ms = sum(ms for k, (_, ms, _) in rec.items() if k == "k_f64_jvp_layer")
            step_ms = sum(ms for k, (_, ms, _) in rec.items() if k.startswith("k_gm64_") and k not in ("k_gm64_backsolve", "k_gm64_combine"))
            fin_calls = sum(c for k, (c, _, _) in rec.items() if k == "k_gm64_finish")
            row.update(profiled_run={"n_iter": int(o["n_iter"]), "n_products": int(o["n_products"]), "product_launches": int(prod_calls),
                                     "arnoldi_steps_launched": int(fin_calls)},
                       fp64_product_us=(1e3 * prod_ms / prod_calls) if prod_calls else None,
                       arnoldi_step_us=(1e3 * step_ms / fin_calls) if fin_calls else None,
                       kernel_ms={k: ms for k, (_, ms, _) in rec.items()})
            print(json.dumps({k: v for k, v in row.items() if k not in ("runs", "kernel_ms")}), flush=True)
            doc["rows"].append(row)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            json.dump(doc, open(args.out, "w"), indent=1)
            nt.close(); fm64.close()
            del nt, fm64, fm32, sv32, o32, o, b, plan, h32, h0_64
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
