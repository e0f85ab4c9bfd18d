"""How far are the fp32 routes of the backward of the VJP (the Jacobian regulariser's double backward) from float64 on large meshes?

The shipped dirichlet and mixed checkpoints (tests/golden/weights_*.npz) on the hexagon meshes of fp64_fixed_point.py (27 361,
101 017, 270 901 and 1 000 519 nodes).  Per mesh, at the state H the model differentiates at (the fp32 device Broyden result at
fw_tol 1e-5 / fw_thres 500 from h0 = encoder(x)), with V = randn (seed 2) and Gbar = 2 J^T V / (N d) -- the cotangent the regulariser
``|V^T J|^2 / (N d)`` puts on ``J^T V``:

* per tensor, the relative L2 against the device's float64 ``FixedPointMap64.vjp_backward`` (``psignn_f64_vjp_backward``) of the fp32
  gather route (``FixedPointMap.vjp_backward``), of the tile route (``tiled=True``) where ``can_tile_vjp_backward()`` holds, and, on
  the dirichlet meshes, of the two-layer chain (a random two-layer block, seed 5, fp32 against float64 at the same H); of ``dH`` too;
* the kernels' own time of the float64 call from the library's launch records (HIP events around every launch), per kernel, and the
  algorithmic bytes stated at the launch sites as a fraction of the HBM peak (8 TB/s);
* the resource usage of the new kernels from profiles/fp64_jr_resource_usage.txt.

One run; nothing is gated.

    python scripts/fp64_vjp_backward.py [--nodes 27000 100000 270000 1000000] [--families dirichlet mixed]
"""
import argparse, importlib, json, os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fp64_derivatives import rel_l2, resource_usage   # noqa: E402
HBM_PEAK_GBS = 8000.0
NOT_MEASURED = "not measured"


def rel(a, b):
    return rel_l2(a, b) if float(b.double().norm()) > 0 else NOT_MEASURED


def flat(named, keys):
    return torch.cat([named[k].reshape(-1) for k in keys])


def two_layer_state_dict(pkg, sd):
    """A random two-layer dirichlet block (seed 5, 1-D tensors N(0, 0.1)) around the checkpoint's encoder and decoder."""
    torch.manual_seed(5)
    net = importlib.import_module("psi-gnn_amd.model_psignn").ModelPSIGNN(dict(latent_dim=10, n_layers=2))
    for q in net.parameters():
        if q.dim() == 1:
            torch.nn.init.normal_(q, std=0.1)
    out = {k: v.detach().clone() for k, v in net.state_dict().items()}
    out.update({k: v for k, v in sd.items() if k.startswith("autoencoder.")})
    return out


def compare(row, tag, got, truth):
    g32, dh32 = got
    g64, dh64 = truth
    row[f"{tag}_rel_l2"] = {k: rel(g32[k], g64[k]) for k in g64}
    row[f"{tag}_rel_l2_flat"] = rel(flat(g32, list(g64)), flat(g64, list(g64)))
    row[f"{tag}_dh_rel_l2"] = rel(dh32, dh64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, nargs="+", default=[27_000, 100_000, 270_000, 1_000_000])
    ap.add_argument("--families", nargs="+", default=["dirichlet", "mixed"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--resource-usage", default=os.path.join(ROOT, "profiles", "fp64_jr_resource_usage.txt"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fp64_vjp_backward.json"))
    args = ap.parse_args()
    pkg = importlib.import_module("psi-gnn_amd"); eng = importlib.import_module("psi-gnn_amd.engine")
    nat = importlib.import_module("psi-gnn_amd._native")
    assert torch.cuda.is_available(), "fp64_vjp_backward.py measures on the GPU"
    dev = torch.device("cuda:0")
    doc = {"settings": {"hbm_peak_gbs": HBM_PEAK_GBS, "reps": args.reps, "runs": 1, "probe": "V = randn(seed 2), Gbar = 2 J^T V / (N d)",
                        "chunk_rows": int(nat.lib().psignn_f64_param_vjp_chunk_rows())},
           "kernels": resource_usage(args.resource_usage) if os.path.exists(args.resource_usage) else NOT_MEASURED, "rows": []}
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
            sv.close()
            H = fw["result"]
            V = torch.randn(H.shape, generator=torch.Generator().manual_seed(2)).to(dev)
            G = (2.0 / H.numel()) * fm64.vjp(H, V)
            row = {"family": family, "n": n, "nodes": plan.N, "tiled": bool(plan.tiled), "forward_lowest": float(fw["lowest"])}
            g64, dh64, jtv = fm64.vjp_backward(H, V, G)
            again = fm64.vjp_backward(H, V, G)
            row["fp64_same_bits_twice"] = bool(all(torch.equal(g64[k], again[0][k]) for k in g64) and torch.equal(dh64, again[1])
                                               and torch.equal(jtv, again[2]))
            row["jac_loss"] = float((jtv * jtv).sum()) / H.numel()
            compare(row, "fp32_gather", fm32.vjp_backward(H, V, G.float()), (g64, dh64))
            if fm32.can_tile_vjp_backward():
                compare(row, "fp32_tiled", fm32.vjp_backward(H, V, G.float(), tiled=True), (g64, dh64))
            else:
                row["fp32_tiled_rel_l2"] = f"{NOT_MEASURED}: can_tile_vjp_backward() is false on this plan"
            # ---- kernel times and bytes of the float64 call
            nat.prof_enable(True); nat.prof_collect()
            for _ in range(args.reps):
                fm64.vjp_backward(H, V, G)
            rec = nat.prof_collect(with_bytes=True); nat.prof_enable(False)
            row["fp64_vjp_backward_kernel_us"] = {k: 1e3 * ms / args.reps for k, (_, ms, _) in rec.items()}
            row["fp64_vjp_backward_us"] = sum(row["fp64_vjp_backward_kernel_us"].values())
            row["fp64_vjp_backward_frac_of_hbm_peak"] = {k: (byts / (ms * 1e-3)) / (HBM_PEAK_GBS * 1e9) if ms > 0 and byts else NOT_MEASURED
                                                         for k, (_, ms, byts) in rec.items()}
            fm64.close()
            # ---- the two-layer chain, dirichlet only (the mixed loop differentiates its last layer alone)
            if not mixed:
                sd2 = two_layer_state_dict(pkg, sd)
                c32 = eng.FixedPointMap(plan, eng.PackedWeights(sd2, dev), h0_64, b.prb_data, nrm)
                c64 = eng.FixedPointMap64(plan, eng.PackedWeights64(sd2), h0_64, b.prb_data, b.edge_attr, nrm)
                G2 = (2.0 / H.numel()) * c64.vjp(H, V)
                t64 = c64.vjp_backward(H, V, G2)
                compare(row, "fp32_two_layer_chain", c32.vjp_backward(H, V, G2.float()), t64[:2])
                c64.close()
                del c32, c64, t64, G2
            print(json.dumps({"family": family, "nodes": plan.N, "same_bits": row["fp64_same_bits_twice"],
                              "gather_flat": row["fp32_gather_rel_l2_flat"], "gather_dh": row["fp32_gather_dh_rel_l2"],
                              "tiled_flat": row.get("fp32_tiled_rel_l2_flat", NOT_MEASURED),
                              "chain_flat": row.get("fp32_two_layer_chain_rel_l2_flat", NOT_MEASURED),
                              "fp64_us": row["fp64_vjp_backward_us"]}), flush=True)
            doc["rows"].append(row)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            json.dump(doc, open(args.out, "w"), indent=1)
            del fm32, fm64, sv, fw, b, plan, H, V, G, g64, dh64, jtv, again
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
