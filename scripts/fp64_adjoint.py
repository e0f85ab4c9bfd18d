"""Is the stall of the fp32 adjoint solves on large meshes fp32 or the method?  The float64 adjoint solves tell.

The shipped dirichlet and mixed checkpoints (tests/golden/weights_*.npz) on the hexagon meshes of fp64_fixed_point.py (27 361,
101 017, 270 901 and 1 000 519 nodes).  Per mesh, at the state H the model differentiates at (the fp32 device Broyden result at
fw_tol 1e-5 / fw_thres 500 from h0 = encoder(x)) and with grad = randn (seed 3), the system y = J_f(H)^T y + grad:

* the float64 restarted GMRES (``DeviceGmres64``, m = 50, eps 1e-11, 2000 products): products, cycles, stop reason, ``lowest``,
  the steps whose second Gram-Schmidt pass ran;
* the float64 Broyden (``DeviceBroyden64.solve_adjoint``, eps 1e-11, threshold 500: 80 GB of pairs at 1M nodes): steps, stop reason,
  ``lowest``, the distance of its result from the float64 GMRES one;
* the fp32 adjoint solves of the same system -- Broyden at bw 1e-8 / 500 and restarted GMRES (m = 50, 500 products) --: what each
  reports and the relative L2 distance of its result from the float64 GMRES result;
* microseconds per float64 product and per Arnoldi step (the ``k_gm64_*`` kernels of a step, the product aside) from the library's
  launch records (HIP events around every launch), with the algorithmic bytes stated at the launch sites as a fraction of the
  HBM peak (8 TB/s);
* the resource usage of the new kernels from profiles/fp64_adjoint_resource_usage.txt.

Nothing is gated.

    python scripts/fp64_adjoint.py [--nodes 27000 100000 270000 1000000] [--families dirichlet mixed] [--out profiles/fp64_adjoint.json]
"""
import argparse, importlib, json, os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fp64_derivatives import rel_l2, resource_usage   # noqa: E402
HBM_PEAK_GBS = 8000.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, nargs="+", default=[27_000, 100_000, 270_000, 1_000_000])
    ap.add_argument("--families", nargs="+", default=["dirichlet", "mixed"])
    ap.add_argument("--m", type=int, default=50)
    ap.add_argument("--max-products", type=int, default=2000)
    ap.add_argument("--threshold", type=int, default=500)
    ap.add_argument("--eps", type=float, default=1e-11)
    ap.add_argument("--resource-usage", default=os.path.join(ROOT, "profiles", "fp64_adjoint_resource_usage.txt"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fp64_adjoint.json"))
    args = ap.parse_args()
    pkg = importlib.import_module("psi-gnn_amd"); eng = importlib.import_module("psi-gnn_amd.engine")
    nat = importlib.import_module("psi-gnn_amd._native")
    assert torch.cuda.is_available(), "fp64_adjoint.py measures on the GPU"
    dev = torch.device("cuda:0")
    doc = {"settings": {"eps": args.eps, "m": args.m, "max_products": args.max_products, "broyden_threshold": args.threshold,
                        "fp32_broyden": "bw 1e-8 / 500", "fp32_gmres": "m 50, 500 products, eps 1e-8", "hbm_peak_GBps": HBM_PEAK_GBS},
           "kernels": resource_usage(args.resource_usage), "rows": []}
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
            fm64 = eng.FixedPointMap64(plan, eng.PackedWeights64(sd), h0_64, b.prb_data, b.edge_attr, nrm)
            sv = eng.DeviceBroyden(plan, threshold=500)
            fw = sv.solve(fm32, 1e-5)
            H = fw["result"]
            grad = torch.randn(H.shape, generator=torch.Generator().manual_seed(3)).to(dev)
            row = {"family": family, "n": n, "nodes": plan.N, "forward_lowest": float(fw["lowest"])}
            # the fp32 solves of the same system
            ob = sv.solve_adjoint(fm32, H, grad, 1e-8)
            sv.close()
            gm32 = eng.DeviceGmres(plan.N * 10, dev, 50)
            og = gm32.solve_adjoint(fm32, H, grad, 1e-8, 500)
            gm32.close()
            y32b, y32g = ob["result"].double(), og["result"].double()
            row.update(fp32_broyden_lowest=float(ob["lowest"]), fp32_broyden_n_iter=int(ob["n_iter"]),
                       fp32_gmres_lowest=float(og["lowest"]), fp32_gmres_products=int(og["nstep"]), fp32_gmres_stop=str(og["stop"]))
            del ob, og, sv, gm32, fm32
            torch.cuda.empty_cache()
            # float64 GMRES, with the library's launch records
            gm = eng.DeviceGmres64(fm64, args.m)
            nat.prof_enable(True); nat.prof_collect()
            g = gm.solve_adjoint(H, grad, args.eps, args.max_products)
            rec = nat.prof_collect(with_bytes=True); nat.prof_enable(False)
            steps = g["nstep"] - (g["n_cycles"] - 1)   # Arnoldi steps: the products that are not a cycle's residual
            prod_ms = sum(ms for k, (_, ms, _) in rec.items() if k.startswith("k_f64_"))
            prod_bytes = sum(by for k, (_, _, by) in rec.items() if k.startswith("k_f64_"))
            step_ms = sum(ms for k, (_, ms, _) in rec.items() if k.startswith("k_gm64_") and k not in ("k_gm64_backsolve", "k_gm64_combine"))
            step_bytes = sum(by for k, (_, _, by) in rec.items() if k.startswith("k_gm64_") and k not in ("k_gm64_backsolve", "k_gm64_combine"))
            row.update(gmres64_products=int(g["nstep"]), gmres64_cycles=int(g["n_cycles"]), gmres64_stop=str(g["stop"]),
                       gmres64_lowest=float(g["lowest"]), gmres64_n_reorth=int(g["n_reorth"]), gmres64_rel_trace=g["rel_trace"],
                       gmres64_bytes=int(gm.nbytes),
                       fp64_product_us=1e3 * prod_ms / max(g["nstep"], 1),
                       fp64_product_frac_of_hbm_peak=(prod_bytes / (prod_ms * 1e-3) / 1e9 / HBM_PEAK_GBS) if prod_ms else None,
                       gmres64_arnoldi_step_us=1e3 * step_ms / max(steps, 1),
                       gmres64_arnoldi_step_frac_of_hbm_peak=(step_bytes / (step_ms * 1e-3) / 1e9 / HBM_PEAK_GBS) if step_ms else None,
                       gmres64_kernel_ms={k: ms for k, (_, ms, _) in rec.items()},
                       fp32_broyden_rel_l2_to_gmres64=rel_l2(y32b, g["result"]), fp32_gmres_rel_l2_to_gmres64=rel_l2(y32g, g["result"]))
            y64 = g["result"]
            gm.close()
            del gm, g
            torch.cuda.empty_cache()
            # float64 Broyden: the reference's own solver in double precision
            try:
                by = eng.DeviceBroyden64(fm64, args.threshold)
                nat.prof_enable(True); nat.prof_collect()
                o = by.solve_adjoint(H, grad, args.eps)
                rec = nat.prof_collect(with_bytes=True); nat.prof_enable(False)
                sweep_ms = sum(ms for k, (_, ms, _) in rec.items() if k.startswith("k_b64_"))
                sweep_bytes = sum(by_ for k, (_, _, by_) in rec.items() if k.startswith("k_b64_"))
                row.update(broyden64_n_iter=int(o["n_iter"]), broyden64_nstep=int(o["nstep"]), broyden64_stop_reason=int(o["stop_reason"]),
                           broyden64_lowest=float(o["lowest"]), broyden64_prot_break=bool(o["prot_break"]), broyden64_bytes=int(by.nbytes),
                           broyden64_rel_l2_to_gmres64=rel_l2(o["result"], y64),
                           broyden64_update_us_per_iter=1e3 * sweep_ms / max(o["n_iter"], 1),
                           broyden64_update_frac_of_hbm_peak=(sweep_bytes / (sweep_ms * 1e-3) / 1e9 / HBM_PEAK_GBS) if sweep_ms else None)
                by.close()
                del by, o
            except nat.NativeError as e:   # the pairs do not fit beside what else the device holds
                row["broyden64_error"] = str(e)
            print(json.dumps(row), flush=True)
            doc["rows"].append(row)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            json.dump(doc, open(args.out, "w"), indent=1)
            fm64.close()
            del fm64, b, plan, H, grad, y64, y32b, y32g, fw
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
