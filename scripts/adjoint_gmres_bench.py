"""The implicit backward's adjoint solve, Broyden against the opt-in restarted GMRES (``bw_solver = "gmres"``): one JSON line.

For each of four routes -- Broyden on the VJP kernels, Broyden on the stored linearisation, GMRES on the VJP kernels, GMRES on the
stored linearisation -- one adjoint solve y = J^T y + grad at bw_tol 1e-8 / bw_thres 500 (the reference's launch configuration):
transposed products, cycles, wall time, launches (psignn_prof_* records of one more, untimed solve) and the bytes of solver state.
The four routes alternate solve by solve in one process, median of ``--reps``.  Sizes: the reference training shape (a union batch of
50 hexagon meshes of 547 nodes: 27 350 nodes), 270 901 nodes and 1 000 519 nodes (``--sizes train,270k,1m`` picks).  H* is the forward
Broyden solve at 1e-5 / 500, grad a seeded Gaussian.  Then one full training step (scripts/train_bench.py's: forward solve, adjoint
solve, parameter-VJP, optimiser; 50-mesh union batch) with the key off and on, alternating, median of ``--steps``.

    python scripts/adjoint_gmres_bench.py [--reps 3] [--steps 5] [--m 50] [--sizes train,270k,1m] [--out profiles/adjoint_gmres_bench.json]"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = lambda n="": importlib.import_module("psi-gnn_amd" + ("." + n if n else ""))
EPS, BUDGET = 1e-8, 500


def weights():
    w = np.load(os.path.join(ROOT, "tests", "golden", "weights_dirichlet.npz"))
    return {k: torch.from_numpy(w[k]) for k in w.files}


def mesh_of(size):
    data = pkg("data")
    if size == "train":
        return data.collate([data.make_hex_problem(13, seed=s, phase=0.37 * s, compute_sol=False) for s in range(50)])
    return data.make_hex_problem({"270k": 300, "1m": 577}[size], seed=0, compute_sol=False)


def solves(size, sd, dev, reps, m):
    eng, nat = pkg("engine"), pkg("_native")
    md = mesh_of(size).to(dev)
    net = pkg("model_psignn").ModelPSIGNN(dict(latent_dim=10, n_layers=1, fw_tol=1e-5, fw_thres=500))
    net.load_state_dict(sd)
    net = net.to(dev).eval()
    with torch.no_grad():
        h0 = net.autoencoder.encoder(md.x)
        fmap = net.deqdss.f.bind(h0, md)
        H = net.deqdss(h0, md)["result"]
    g = torch.randn(H.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(0))
    lin = fmap.linearize_p(fmap.to_plan(H))
    bro = eng.DeviceBroyden(plan=fmap.plan, threshold=BUDGET, keep_trace=False)
    gm = eng.DeviceGmres(fmap.plan.N * 10, dev, m)
    routes = {"broyden_direct": lambda: bro.solve_adjoint(fmap, H, g, EPS),
              "broyden_lin": lambda: bro.solve_adjoint(fmap, H, g, EPS, lin=lin),
              "gmres_direct": lambda: gm.solve_adjoint(fmap, H, g, EPS, BUDGET),
              "gmres_lin": lambda: gm.solve_adjoint(fmap, H, g, EPS, BUDGET, lin=lin)}
    outs = {k: f() for k, f in routes.items()}   # warm-up: workspaces, transposed masks
    torch.cuda.synchronize()
    times = {k: [] for k in routes}
    for _ in range(reps):
        for k, f in routes.items():
            t0 = time.perf_counter()
            outs[k] = f()
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t0)
    rows = {}
    nat.prof_enable(True)
    for k, f in routes.items():
        nat.prof_collect()
        f()
        rec = nat.prof_collect()
        o = outs[k]
        is_gm = k.startswith("gmres")
        rows[k] = {"products": int(o["nstep"] if is_gm else o["n_iter"]), "cycles": int(o["n_cycles"]) if is_gm else None,
                   "stop": o["stop"] if is_gm else int(o["stop_reason"]), "lowest": float(o["lowest"]),
                   "ms_median": 1e3 * statistics.median(times[k]), "ms_all": [1e3 * t for t in times[k]],
                   "launches": int(sum(v[0] for v in rec.values())),
                   "top_ms": {q: round(v[1], 3) for q, v in sorted(rec.items(), key=lambda kv: -kv[1][1])[:6]},
                   "solver_state_bytes": int(gm.nbytes if is_gm else bro.nbytes)}
    nat.prof_enable(False)
    ref = outs["broyden_lin"]["result"]
    for k in rows:
        rows[k]["rel_l2_vs_broyden_lin"] = float((outs[k]["result"] - ref).norm() / ref.norm())
    res = {"N": int(fmap.plan.N), "m": m, "bw_tol": EPS, "bw_thres": BUDGET, "routes": rows,
           "gmres_lin_over_broyden_lin": rows["gmres_lin"]["ms_median"] / rows["broyden_lin"]["ms_median"],
           "gmres_direct_over_broyden_direct": rows["gmres_direct"]["ms_median"] / rows["broyden_direct"]["ms_median"]}
    for o in (lin, bro, gm):
        o.close()
    return res


def train_steps(sd, dev, steps, m):
    """One full training step on the reference training shape with the key off and on (both with the stored linearisation, the faster
    backward of either solver), alternating."""
    solver, TrainModel, nat = pkg("utilities.solver"), pkg("training_class").TrainModel, pkg("_native")
    bd = mesh_of("train").to(dev)

    def trainer(**kw):
        cfg = dict(latent_dim=10, n_layers=1, solver=solver.broyden, fw_tol=1e-5, fw_thres=500, bw_tol=EPS, bw_thres=BUDGET,
                   bw_linearize=True, **kw)
        net = pkg("model_psignn").ModelDEQDSS(cfg)
        net.load_state_dict(sd)
        net = net.to(dev).train()
        return TrainModel(dict(loader_train=[], loader_val=[], model=net, config_model=net.config, lr_deq=1e-6, lr_ae=1e-6,
                               sched_step_deq=0.5, sched_step_ae=0.5, path_ckpt=None, min_loss_save=1e9, max_epochs=0,
                               gradient_clip=1e-2, sup_weight=0.0, jac_weight=1.0))

    trs = {"key_off": trainer(), "key_on": trainer(bw_solver="gmres", bw_gmres_m=m)}
    for t in trs.values():
        t.train_step(bd)
    torch.cuda.synchronize()
    times = {k: [] for k in trs}
    for _ in range(steps):
        for k, t in trs.items():
            t0 = time.perf_counter()
            t.train_step(bd)
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t0)
    out = {"workload": f"training step, union batch of 50 hexagon meshes (n=13): {bd.num_nodes} nodes; fw 1e-5 / 500, bw 1e-8 / 500, "
                       f"bw_linearize, jac_weight 1", "steps": steps}
    nat.prof_enable(True)
    for k, t in trs.items():
        nat.prof_collect()
        t.train_step(bd)
        torch.cuda.synchronize()
        rec = nat.prof_collect()
        bw = t.net.deqdss.last_backward
        out[k] = {"s_per_step_median": statistics.median(times[k]), "s_per_step_all": times[k],
                  "bw_products": int(bw["nstep"] if "n_cycles" in bw else bw["n_iter"]), "bw_lowest": float(bw["lowest"]),
                  "launches": int(sum(v[0] for v in rec.values()))}
    nat.prof_enable(False)
    out["key_on_over_key_off"] = out["key_on"]["s_per_step_median"] / out["key_off"]["s_per_step_median"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--m", type=int, default=50)
    ap.add_argument("--sizes", default="train,270k,1m")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    sd = weights()
    res = {"device": torch.cuda.get_device_name(0),
           "timing": "wall clock around one synchronised call, the routes alternating call by call after one warm call of each; median"}
    for size in a.sizes.split(","):
        if size:
            res["solve_" + size] = solves(size, sd, dev, a.reps, a.m)
    if a.steps > 0:
        res["train_step"] = train_steps(sd, dev, a.steps, a.m)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
