"""How far is the fp32 training step from float64 on large meshes, with the cotangent a training loss really produces?

The shipped dirichlet and mixed checkpoints (tests/golden/weights_*.npz) on the hexagon meshes of fp64_fixed_point.py (27 361,
101 017, 270 901 and 1 000 519 nodes), ``sol`` from ``compute_sol="device"``.  Per mesh:

* the fp32 training step: ``ModelDEQDSS`` in train mode (fw 1e-5 / 500, bw 1e-8 / 500), loss = residual + 1.0 jacobian + encoder +
  autoencoder, ``loss.backward()``;
* ``engine.train_step64`` at its own ``h*`` (``last_forward``), ``y`` (``last_backward``) and probe (``last_probe``): per tensor the
  relative L2 of the fp32 gradient against the float64 one, the flat vector too, and the loss terms of both;
* the float64 gradient at the float64 GMRES ``y`` for the same ``grad_h`` (``implicit_grad64``: eps 1e-11, m 50, 2000 products): how far
  the fp32 adjoint's ``y`` and the gradient that follows from it are from the converged float64 adjoint -- the question of DESIGN
  section 7-3b asked with a loss cotangent instead of randn;
* the wall time of the float64 call at a given state (one call after a warm-up call, device synchronised) and the new kernels' own
  time from the library's launch records, with the algorithmic bytes stated at their launch sites as a fraction of the HBM peak.

One run; nothing is gated.  Rows are appended to the output file, so that every mesh can run as a process of its own under its own
time limit:

    python scripts/fp64_train_step.py [--nodes 27000 100000 270000 1000000] [--families dirichlet mixed] [--fresh]
"""
import argparse, importlib, json, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fp64_derivatives import rel_l2, resource_usage   # noqa: E402
HBM_PEAK_GBS = 8000.0
NOT_MEASURED = "not measured"
NEW_KERNELS = ("k_residual_f64", "k_residual_t_f64", "k_mse_f64", "k_mse_f64_final")


def rel(a, b):
    return rel_l2(a, b) if float(b.double().norm()) > 0 else NOT_MEASURED


def flat(named, keys):
    return torch.cat([named[k].reshape(-1).double() for k in keys])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, nargs="+", default=[27_000, 100_000, 270_000, 1_000_000])
    ap.add_argument("--families", nargs="+", default=["dirichlet", "mixed"])
    ap.add_argument("--fresh", action="store_true", help="start the output file anew instead of appending rows to it")
    ap.add_argument("--resource-usage", default=os.path.join(ROOT, "profiles", "fp64_loss_resource_usage.txt"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fp64_train_step.json"))
    args = ap.parse_args()
    pkg = importlib.import_module("psi-gnn_amd"); eng = importlib.import_module("psi-gnn_amd.engine")
    nat = importlib.import_module("psi-gnn_amd._native"); solver = importlib.import_module("psi-gnn_amd.utilities.solver")
    assert torch.cuda.is_available(), "fp64_train_step.py measures on the GPU"
    dev = torch.device("cuda:0")
    if os.path.exists(args.out) and not args.fresh:
        doc = json.load(open(args.out))
    else:
        doc = {"settings": {"hbm_peak_gbs": HBM_PEAK_GBS, "runs": 1, "jac_weight": 1.0, "fp32": "fw 1e-5 / 500, bw 1e-8 / 500",
                            "float64_adjoint": "gmres, eps 1e-11, m 50, 2000 products", "mse_chunk": int(nat.lib().psignn_mse_f64_chunk())},
               "kernels": resource_usage(args.resource_usage) if os.path.exists(args.resource_usage) else NOT_MEASURED, "rows": []}
    for family in args.families:
        mixed = family == "mixed"
        w = np.load(os.path.join(ROOT, "tests", "golden", f"weights_{family}.npz")); sd = {k: torch.from_numpy(w[k]) for k in w.files}
        for target in args.nodes:
            n = pkg.data.hex_n_for_nodes(target)
            b = pkg.data.make_hex_problem(n, seed=0, mixed=mixed, compute_sol="device").to(dev)
            cfg = dict(latent_dim=10, n_layers=1, solver=solver.broyden, fw_tol=1e-5, fw_thres=500, bw_tol=1e-8, bw_thres=500)
            net = importlib.import_module("psi-gnn_amd.mixed" if mixed else "psi-gnn_amd.model_psignn").ModelDEQDSS(cfg)
            net.load_state_dict(sd); net = net.to(dev).train()
            torch.manual_seed(2)
            u, ld = net(b)
            (ld["residual_loss"] + 1.0 * ld["jacobian_loss"] + ld["encoder_loss"] + ld["autoencoder_loss"]).backward()
            got = {k: p.grad.detach() for k, p in net.named_parameters()}
            deq = net.deqdss
            hs, y, probe = deq.last_forward["result"], deq.last_backward["result"], deq.last_probe
            row = {"family": family, "n": n, "nodes": int(b.x.shape[0]), "fp32_forward_lowest": float(deq.last_forward["lowest"]),
                   "fp32_forward_nstep": int(deq.last_forward["nstep"]), "fp32_backward_lowest": float(deq.last_backward["lowest"]),
                   "fp32_backward_nstep": int(deq.last_backward["nstep"])}
            eng.train_step64(b, sd, h_star=hs, y=y, probe=probe, jac_weight=1.0)   # warm-up: plans, workspaces
            torch.cuda.synchronize(dev); t0 = time.perf_counter()
            nat.prof_enable(True); nat.prof_collect()
            t64 = eng.train_step64(b, sd, h_star=hs, y=y, probe=probe, jac_weight=1.0)
            torch.cuda.synchronize(dev); row["train_step64_given_state_wall_ms"] = 1e3 * (time.perf_counter() - t0)
            rec = nat.prof_collect(with_bytes=True); nat.prof_enable(False)
            row["new_kernel_us"] = {k: 1e3 * rec[k][1] / rec[k][0] for k in NEW_KERNELS if k in rec}
            row["new_kernel_calls"] = {k: rec[k][0] for k in NEW_KERNELS if k in rec}
            row["new_kernel_frac_of_hbm_peak"] = {k: (rec[k][2] / (rec[k][1] * 1e-3)) / (HBM_PEAK_GBS * 1e9) if rec[k][1] > 0 and rec[k][2]
                                                  else NOT_MEASURED for k in NEW_KERNELS if k in rec}
            row["all_kernel_us_of_the_call"] = sum(1e3 * ms for _, ms, _ in rec.values())
            g64 = t64["grads"]
            row["loss_terms_fp32"] = {k: float(v.detach()) for k, v in ld.items() if torch.is_tensor(v) and v.numel() == 1}
            row["loss_terms_float64"] = t64["loss_dic"]
            row["fp32_rel_l2"] = {k: rel(got[k], g64[k]) for k in g64}
            row["fp32_rel_l2_flat"] = rel(flat(got, list(g64)), flat(g64, list(g64)))
            # ---- the same grad_h with the float64 adjoint converged: what the fp32 adjoint solve costs the gradient
            imp = eng.implicit_grad64(b, sd, hs, t64["grad_h"])
            adj = imp["adjoint"]
            row["float64_adjoint"] = {"products": int(adj["nstep"]), "lowest": float(adj["lowest"]), "stop": adj["stop"]}
            row["fp32_y_rel_l2_to_float64_y"] = rel(y, imp["y"])
            keys = list(imp["grads"])
            at32 = eng.implicit_grad64(b, sd, hs, t64["grad_h"], y=y)["grads"]   # the implicit part alone, at the fp32 y
            row["implicit_part_at_fp32_y_rel_l2_to_float64_y"] = {k: rel(at32[k], imp["grads"][k]) for k in keys}
            row["implicit_part_at_fp32_y_rel_l2_flat"] = rel(flat(at32, keys), flat(imp["grads"], keys))
            print(json.dumps({"family": family, "nodes": row["nodes"], "fp32_flat": row["fp32_rel_l2_flat"],
                              "worst_tensor": max(((v, k) for k, v in row["fp32_rel_l2"].items() if not isinstance(v, str)), default=None),
                              "y32_vs_y64": row["fp32_y_rel_l2_to_float64_y"], "implicit_flat": row["implicit_part_at_fp32_y_rel_l2_flat"],
                              "gmres": row["float64_adjoint"], "wall_ms": row["train_step64_given_state_wall_ms"],
                              "new_kernel_us": row["new_kernel_us"]}), flush=True)
            doc["rows"].append(row)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            json.dump(doc, open(args.out, "w"), indent=1)
            del net, b, t64, imp, at32, got, hs, y, probe
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
