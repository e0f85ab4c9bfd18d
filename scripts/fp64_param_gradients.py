"""How far are the fp32 parameter-gradient kernels from float64 on large meshes, and does the stall of the adjoint solves (DESIGN.md
sections 7-3b and 7-4) move the training gradient?

The shipped dirichlet and mixed checkpoints (tests/golden/weights_*.npz) on the hexagon meshes of fp64_fixed_point.py (27 361,
101 017, 270 901 and 1 000 519 nodes).  Per mesh, at the state H the model differentiates at (the fp32 device Broyden result at
fw_tol 1e-5 / fw_thres 500 from h0 = encoder(x)):

* with w = randn (seed 2): per tensor, the relative L2 of the fp32 ``FixedPointMap.param_vjp_init`` against the device's float64
  ``FixedPointMap64.param_vjp`` (``psignn_f64_param_vjp``); of ``J^T w`` and ``dH_init`` too;
* the kernels' own time of the float64 call from the library's launch records (HIP events around every launch), per kernel, and the
  algorithmic bytes stated at the launch sites as a fraction of the HBM peak (8 TB/s);
* with grad = randn (seed 3), the system y = J_f(H)^T y + grad solved four ways -- fp32 Broyden (bw 1e-8 / 500), fp32 restarted GMRES
  (m = 50, 500 products), float64 GMRES (m = 50, eps 1e-11, 2000 products), float64 Broyden (eps 1e-11, threshold 500) -- and the
  float64 parameter gradient ``param_vjp(H, y)`` at each y: relative L2 and cosine between the gradients, per tensor and for the whole
  flat vector, every pair of solves; the distance between the y themselves beside them.  That is the answer to "does the adjoint
  stall move the gradient";
* the resource usage of the new kernels from profiles/fp64_pgrad_resource_usage.txt.

Nothing is gated.

    python scripts/fp64_param_gradients.py [--nodes 27000 100000 270000 1000000] [--families dirichlet mixed]
"""
import argparse, importlib, itertools, json, os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fp64_derivatives import rel_l2, resource_usage   # noqa: E402
HBM_PEAK_GBS = 8000.0
NOT_MEASURED = "not measured"


def cosine(a, b):
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    d = float(a.norm() * b.norm())
    return float((a * b).sum()) / d if d > 0 else NOT_MEASURED


def rel(a, b):
    return rel_l2(a, b) if float(b.double().norm()) > 0 else NOT_MEASURED


def flat(named):
    return torch.cat([t.reshape(-1) for t in named.values()])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, nargs="+", default=[27_000, 100_000, 270_000, 1_000_000])
    ap.add_argument("--families", nargs="+", default=["dirichlet", "mixed"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threshold", type=int, default=500)
    ap.add_argument("--resource-usage", default=os.path.join(ROOT, "profiles", "fp64_pgrad_resource_usage.txt"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fp64_param_gradients.json"))
    args = ap.parse_args()
    pkg = importlib.import_module("psi-gnn_amd"); eng = importlib.import_module("psi-gnn_amd.engine")
    nat = importlib.import_module("psi-gnn_amd._native")
    assert torch.cuda.is_available(), "fp64_param_gradients.py measures on the GPU"
    dev = torch.device("cuda:0")
    doc = {"settings": {"hbm_peak_gbs": HBM_PEAK_GBS, "reps": args.reps, "chunk_rows": int(nat.lib().psignn_f64_param_vjp_chunk_rows()),
                        "fp32_broyden": "bw 1e-8 / 500", "fp32_gmres": "m 50, 500 products", "gmres64": "m 50, eps 1e-11, 2000 products",
                        "broyden64": f"eps 1e-11, threshold {args.threshold}"},
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
            rnd = lambda seed: torch.randn(H.shape, generator=torch.Generator().manual_seed(seed)).to(dev)
            wv, grad = rnd(2), rnd(3)
            row = {"family": family, "n": n, "nodes": plan.N, "tiled": bool(plan.tiled), "forward_lowest": float(fw["lowest"])}
            # ---- the fp32 kernels against float64, w = randn
            g32, dh32, di32 = fm32.param_vjp_init(H, wv)
            g64, dh64, di64 = fm64.param_vjp(H, wv)
            again = fm64.param_vjp(H, wv)
            row["fp64_same_bits_twice"] = bool(all(torch.equal(g64[k], again[0][k]) for k in g64) and torch.equal(dh64, again[1]))
            row["fp32_param_vjp_rel_l2"] = {k: rel(g32[k], g64[k]) for k in g64}
            row["fp32_param_vjp_rel_l2_flat"] = rel(flat({k: g32[k] for k in g64}), flat(g64))
            row["fp32_dh_rel_l2"], row["fp32_dh_init_rel_l2"] = rel(dh32, dh64), rel(di32, di64)
            # ---- kernel times and bytes of the float64 call
            nat.prof_enable(True); nat.prof_collect()
            for _ in range(args.reps):
                fm64.param_vjp(H, wv)
            rec = nat.prof_collect(with_bytes=True); nat.prof_enable(False)
            row["fp64_param_vjp_kernel_us"] = {k: 1e3 * ms / args.reps for k, (_, ms, _) in rec.items()}
            row["fp64_param_vjp_us"] = sum(row["fp64_param_vjp_kernel_us"].values())
            row["fp64_param_vjp_frac_of_hbm_peak"] = {k: (byts / (ms * 1e-3)) / (HBM_PEAK_GBS * 1e9) if ms > 0 and byts else NOT_MEASURED
                                                      for k, (_, ms, byts) in rec.items()}
            # ---- the same float64 gradient at four adjoint solutions
            ys, info = {}, {}
            ob = sv.solve_adjoint(fm32, H, grad, 1e-8)
            ys["fp32_broyden"], info["fp32_broyden"] = ob["result"], {"lowest": float(ob["lowest"]), "n_iter": int(ob["n_iter"])}
            sv.close()
            gm = eng.DeviceGmres(plan.N * 10, dev, 50)
            og = gm.solve_adjoint(fm32, H, grad, 1e-8, 500)
            ys["fp32_gmres"], info["fp32_gmres"] = og["result"], {"lowest": float(og["lowest"]), "products": int(og["nstep"]),
                                                                  "stop": str(og["stop"])}
            gm.close()
            g6 = eng.DeviceGmres64(fm64, 50)
            o6 = g6.solve_adjoint(H, grad, 1e-11, 2000)
            ys["gmres64"], info["gmres64"] = o6["result"], {"lowest": float(o6["lowest"]), "products": int(o6["nstep"]),
                                                            "stop": str(o6["stop"])}
            g6.close()
            try:
                b6 = eng.DeviceBroyden64(fm64, args.threshold)
                ob6 = b6.solve_adjoint(H, grad, 1e-11)
                ys["broyden64"], info["broyden64"] = ob6["result"], {"lowest": float(ob6["lowest"]), "n_iter": int(ob6["n_iter"]),
                                                                     "nstep": int(ob6["nstep"])}
                b6.close()
                del b6, ob6
            except nat.NativeError as e:   # the pairs did not fit
                info["broyden64"] = f"{NOT_MEASURED}: {e}"
            torch.cuda.empty_cache()
            row["adjoint_solves"] = info
            grads = {k: fm64.param_vjp(H, y, with_init=False)[0] for k, y in ys.items()}
            pairs = {}
            for a, c in itertools.combinations(grads, 2):
                pairs[f"{a} vs {c}"] = {
                    "y_rel_l2": rel(ys[a], ys[c]), "y_cosine": cosine(ys[a], ys[c]),
                    "grad_rel_l2_flat": rel(flat(grads[a]), flat(grads[c])), "grad_cosine_flat": cosine(flat(grads[a]), flat(grads[c])),
                    "grad_rel_l2": {k: rel(grads[a][k], grads[c][k]) for k in grads[c]},
                    "grad_cosine": {k: cosine(grads[a][k], grads[c][k]) for k in grads[c]}}
            row["gradient_at_adjoint_solutions"] = pairs
            worst = {p: max((v for v in d["grad_rel_l2"].values() if v != NOT_MEASURED), default=NOT_MEASURED) for p, d in pairs.items()}
            print(json.dumps({"family": family, "nodes": plan.N, "fp32_flat": row["fp32_param_vjp_rel_l2_flat"],
                              "fp64_us": row["fp64_param_vjp_us"], "same_bits": row["fp64_same_bits_twice"],
                              "pairs_flat": {p: (d["y_rel_l2"], d["grad_rel_l2_flat"], d["grad_cosine_flat"]) for p, d in pairs.items()},
                              "pairs_worst_tensor": worst}), flush=True)
            doc["rows"].append(row)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            json.dump(doc, open(args.out, "w"), indent=1)
            fm64.close()
            del fm32, fm64, sv, gm, g6, fw, ob, og, o6, b, plan, H, wv, grad, ys, grads, g32, g64, dh32, dh64, di32, di64, again
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
