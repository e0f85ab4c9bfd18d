"""How far are the fp32 derivative kernels, and the fp32 adjoint solves, from float64 on large meshes?

The shipped dirichlet and mixed checkpoints (tests/golden/weights_*.npz) on the hexagon meshes of fp64_fixed_point.py (27 361,
101 017, 270 901 and 1 000 519 nodes).  Per mesh, at the state H the model differentiates at (the fp32 device Broyden result at
fw_tol 1e-5 / fw_thres 500 from h0 = encoder(x)) and with v, w, grad = randn (seeds 1, 2, 3):

* relative L2 of the fp32 ``FixedPointMap.jvp`` / ``.vjp`` and of the stored linearisation's ``jvp_p`` / ``vjp_p`` against the
  device's float64 products ``FixedPointMap64.jvp`` / ``.vjp`` (``psignn_f64_jvp`` / ``psignn_f64_vjp``);
* how many rows of each fp32 product are off by more than 1e-5 of the RMS row norm, and the relative L2 over the other rows (a
  ReLU mask that differs from the float64 one is an O(1) error on a few rows; rounding is ~1e-7 on all of them);
* the duality gap |<w, J v> - <J^T w, v>| / |<w, J v>| of the float64 products;
* the fp32 adjoint solves of y = J^T y + grad -- Broyden at bw 1e-8 / 500 and restarted GMRES (m = 50, 500 products) --: the measure
  each reports, and the same measure |f(y) - y| / (|f(y)| + 1e-9) of its result recomputed with the float64 map
  f(y) = ``FixedPointMap64.vjp(H, y, grad)``;
* microseconds per float64 product, twice: the host clock around ``--reps`` back-to-back ``FixedPointMap64`` calls (that includes
  the output allocation and the Python / ctypes call, a visible share on the small meshes), and the kernels' own time from the
  library's launch records (HIP events around every launch);
* VGPRs / scratch / occupancy of the float64 derivative kernels, parsed from the compiler's ``-Rpass-analysis=kernel-resource-usage``
  remarks (``--resource-usage``, default profiles/fp64_deriv_resource_usage.txt).

Nothing is gated.  This script predates the float64 adjoint solves and records their steps, their ``lowest`` and the distance of
the fp32 adjoint solutions from them as "not measured"; scripts/fp64_adjoint.py measures those.

    python scripts/fp64_derivatives.py [--nodes 27000 100000 270000 1000000] [--out profiles/fp64_derivatives.json]
"""
import argparse, importlib, json, os, re, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
NOT_MEASURED = "not measured"


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def row_errors(got, want, factor=1e-5):
    """(rows whose error norm exceeds ``factor`` x the RMS row norm of ``want``, relative L2 over the other rows): an fp32 ReLU
    mask that differs from the float64 one puts an O(1) error on a few rows, rounding puts ~1e-7 on all of them."""
    d, wd = (got.double() - want).norm(dim=1), want.norm(dim=1)
    off = d > factor * float(wd.pow(2).mean().sqrt())
    keep = ~off
    return int(off.sum()), float(d[keep].norm() / wd[keep].norm())


def resource_usage(path):
    """{kernel: {vgprs, scratch_bytes_per_lane, occupancy}} from the remarks of one compile of csrc/fgnn_f64_deriv.hip."""
    if not os.path.exists(path):
        return NOT_MEASURED
    out, cur = {}, None
    for line in open(path):
        m = re.search(r"remark:\s+(Function Name|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\S+)", line)
        if not m:
            continue
        key, val = m.groups()
        if key == "Function Name":
            cur = out.setdefault(val, {})
        elif cur is not None:
            cur[{"VGPRs": "vgprs", "ScratchSize [bytes/lane]": "scratch_bytes_per_lane", "Occupancy [waves/SIMD]": "occupancy"}[key]] = int(val)
    return out


def timed_us(fn, reps):
    fn(); torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return 1e6 * (time.perf_counter() - t0) / reps


def kernel_us(nat, fn, reps):
    """Microseconds of the library's kernels per call of ``fn``, from its own launch records (HIP events around every launch):
    {kernel name: us per call} and their sum -- the device time, without the host's share of ``timed_us``."""
    fn(); torch.cuda.synchronize()
    nat.prof_enable(True); nat.prof_collect()
    for _ in range(reps):
        fn()
    rec = nat.prof_collect(); nat.prof_enable(False)
    per = {k: 1e3 * ms / reps for k, (_, ms) in rec.items()}
    return per, sum(per.values())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, nargs="+", default=[27_000, 100_000, 270_000, 1_000_000])
    ap.add_argument("--families", nargs="+", default=["dirichlet", "mixed"])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--resource-usage", default=os.path.join(ROOT, "profiles", "fp64_deriv_resource_usage.txt"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fp64_derivatives.json"))
    args = ap.parse_args()
    pkg = importlib.import_module("psi-gnn_amd"); eng = importlib.import_module("psi-gnn_amd.engine")
    nat = importlib.import_module("psi-gnn_amd._native")
    assert torch.cuda.is_available(), "fp64_derivatives.py measures on the GPU"
    dev = torch.device("cuda:0")
    doc = {"kernels": resource_usage(args.resource_usage), "fp64_adjoint_solve": NOT_MEASURED, "rows": []}
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
            v, wv, grad = rnd(1), rnd(2), rnd(3)
            jv64, jtw64 = fm64.jvp(H, v), fm64.vjp(H, wv)
            a, c = float((wv.double() * jv64).sum()), float((jtw64 * v.double()).sum())
            jv32, jtw32 = fm32.jvp(H, v), fm32.vjp(H, wv)
            row = {"family": family, "n": n, "nodes": plan.N, "tiled": bool(plan.tiled), "forward_lowest": float(fw["lowest"]),
                   "fp32_jvp_rel_l2": rel_l2(jv32, jv64), "fp32_vjp_rel_l2": rel_l2(jtw32, jtw64),
                   "fp64_duality_gap": abs(a - c) / abs(a)}
            row["fp32_jvp_rows_off"], row["fp32_jvp_rel_l2_other_rows"] = row_errors(jv32, jv64)
            row["fp32_vjp_rows_off"], row["fp32_vjp_rel_l2_other_rows"] = row_errors(jtw32, jtw64)
            if fm32.can_linearize():
                lin = fm32.linearize_p(fm32.to_plan(H))
                row["lin_jvp_p_rel_l2"] = rel_l2(fm32.from_plan(lin.jvp_p(fm32.to_plan(v))), jv64)
                row["lin_vjp_p_rel_l2"] = rel_l2(fm32.from_plan(lin.vjp_p(fm32.to_plan(wv))), jtw64)
                lin.close()
            else:
                row["lin_jvp_p_rel_l2"] = row["lin_vjp_p_rel_l2"] = NOT_MEASURED

            def measure64(y):   # the adjoint system's stop measure at y, in float64
                f = fm64.vjp(H, y, grad)
                return float((f - y.double()).norm() / (f.norm() + 1e-9))
            ob = sv.solve_adjoint(fm32, H, grad, 1e-8)
            row.update(fp32_broyden_adjoint_lowest=float(ob["lowest"]), fp32_broyden_adjoint_n_iter=int(ob["n_iter"]),
                       fp32_broyden_adjoint_measure_in_fp64=measure64(ob["result"]))
            sv.close()
            gm = eng.DeviceGmres(plan.N * 10, dev, 50)
            og = gm.solve_adjoint(fm32, H, grad, 1e-8, 500)
            row.update(fp32_gmres_adjoint_lowest=float(og["lowest"]), fp32_gmres_adjoint_products=int(og["nstep"]),
                       fp32_gmres_adjoint_stop=str(og["stop"]), fp32_gmres_adjoint_measure_in_fp64=measure64(og["result"]),
                       fp32_broyden_vs_gmres_adjoint_rel_l2=rel_l2(ob["result"], og["result"]))
            gm.close()
            jk, jsum = kernel_us(nat, lambda: fm64.jvp(H, v), args.reps)
            vk, vsum = kernel_us(nat, lambda: fm64.vjp(H, wv), args.reps)
            row.update(fp64_jvp_us=timed_us(lambda: fm64.jvp(H, v), args.reps), fp64_vjp_us=timed_us(lambda: fm64.vjp(H, wv), args.reps),
                       fp64_jvp_kernel_us=jsum, fp64_vjp_kernel_us=vsum, fp64_kernel_us={**jk, **vk},
                       fp64_adjoint_steps=NOT_MEASURED, fp64_adjoint_lowest=NOT_MEASURED, fp64_adjoint_us_per_iter=NOT_MEASURED,
                       fp32_broyden_adjoint_rel_l2_to_fp64=NOT_MEASURED, fp32_gmres_adjoint_rel_l2_to_fp64=NOT_MEASURED)
            print(json.dumps(row), flush=True)
            doc["rows"].append(row)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            json.dump(doc, open(args.out, "w"), indent=1)
            fm64.close()
            del fm32, fm64, sv, gm, fw, ob, og, b, plan, H, v, wv, grad, jv64, jtw64, jv32, jtw32
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
