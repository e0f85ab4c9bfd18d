"""Training-step timing: one optimisation step of the dirichlet model on a union batch of synthetic
hexagon meshes -- forward Broyden solve, on-device adjoint solve, parameter-VJP, optimiser -- on the HIP path, with
the CPU oracle's restated training step (autograd + restated broyden) timed beside it on the same batch.

    python3 scripts/train_bench.py [graphs_per_batch=50] [hex_n=13] [steps=5] [cpu=1] [jac_weight=0] [family=dirichlet|mixed] [replicas=R]
                                   [bw_solver=gmres] [lockstep=1]

replicas=R (anywhere on the line): R union batches of graphs_per_batch graphs each.  One step over the R batches as replicas in
lockstep (``net(list_of_batches)``: batched forward and adjoint solves, the reference's ``DataParallel`` with ``num_gpus = R``) is
timed beside R sequential single-batch steps over the same batches -- the single-batch route as it is without the option, and the
same with ``bw_linearize`` (the lockstep's backward is always the linearised one) --, the three alternated step by step in one
process, median of ``steps``.  Every sequential route keeps one model per batch, so that no route re-allocates solver state
between steps.  The CPU oracle is not timed in this mode.  route=lockstep|sequential|sequential_lin restricts the run to one route
(a profiler run of that route in a process of its own).  bw_solver=gmres (with replicas=R): every route's implicit backward is the
restarted GMRES solve (``bw_solver = "gmres"``); the replica step then solves its replicas one after the other unless lockstep=1
is given too (``bw_gmres_lockstep = True``: the GMRES adjoint solves of the replicas in lockstep).

jac_weight = 1 is what the reference's launch scripts use (launch_local.sh:24): the step then also runs the backward of
the VJP (csrc/gather_backward.hip).

The reference trains on ~500-node meshes (hsize 0.08) in PyG batches; hex_n = 13 gives 547 nodes per graph.
Prints one JSON line."""
import importlib
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = lambda n="": importlib.import_module("psi-gnn_amd" + ("." + n if n else ""))


def replicas_main(argv, R, only=None, bw_solver=None, gmres_lockstep=False):
    import statistics
    import numpy as np
    B = int(argv[1]) if len(argv) > 1 else 50
    n = int(argv[2]) if len(argv) > 2 else 13
    steps = int(argv[3]) if len(argv) > 3 else 5
    jw = float(argv[5]) if len(argv) > 5 else 0.0
    mixed = len(argv) > 6 and argv[6] == "mixed"
    data, nat = pkg("data"), pkg("_native")
    w = np.load(os.path.join(ROOT, "tests", "golden", "weights_mixed.npz" if mixed else "weights_dirichlet.npz"))
    sd = {k: torch.from_numpy(w[k]) for k in w.files}
    dev = torch.device("cuda:0")
    batches = [data.collate([data.make_hex_problem(n, seed=r * B + s, phase=0.37 * (r * B + s), mixed=mixed, compute_sol=False)
                             for s in range(B)]).to(dev) for r in range(R)]   # (no LU solution: mse_loss is only a statistic here)
    solver = pkg("utilities.solver")
    TrainModel = pkg("training_class").TrainModel

    def trainer(**kw):
        cfg = dict(latent_dim=10, n_layers=1, solver=solver.broyden, fw_tol=1e-5, fw_thres=500, bw_tol=1e-8, bw_thres=500, **kw)
        if bw_solver is not None:
            cfg["bw_solver"] = bw_solver
        if mixed:
            cfg["lin_neumann"] = "stored"
        net = (pkg("mixed") if mixed else pkg("model_psignn")).ModelDEQDSS(cfg)
        net.load_state_dict(sd)
        net = net.to(dev).train()
        return TrainModel(dict(loader_train=[], loader_val=[], model=net, config_model=net.config, lr_deq=1e-6, lr_ae=1e-6,
                               sched_step_deq=0.5, sched_step_ae=0.5, path_ckpt=None, min_loss_save=1e9, max_epochs=0,
                               gradient_clip=1e-2, sup_weight=0.0, jac_weight=jw))

    lock = trainer(**({"bw_gmres_lockstep": True, "bw_linearize": True} if gmres_lockstep else {})) if only in (None, "lockstep") else None
    seq = [trainer() for _ in range(R)] if only in (None, "sequential") else []
    seq_lin = [trainer(bw_linearize=True) for _ in range(R)] if only in (None, "sequential_lin") else []
    routes = {"lockstep": lambda: lock.train_step(batches),
              "sequential": lambda: [t.train_step(b) for t, b in zip(seq, batches)],
              "sequential_lin": lambda: [t.train_step(b) for t, b in zip(seq_lin, batches)]}
    if only is not None:
        routes = {only: routes[only]}
    times = {k: [] for k in routes}
    for k, f in routes.items():   # warm-up (plan build, allocations); lr = 1e-6 keeps the weights at the checkpoint
        f()
    torch.cuda.synchronize()
    for _ in range(steps):
        for k, f in routes.items():
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t0)
    kern = {}
    nat.prof_enable(True)
    for k, f in routes.items():   # one more step of each with the library's per-kernel records (not timed)
        nat.prof_collect()
        f()
        torch.cuda.synchronize()
        rec = nat.prof_collect()
        kern[k] = {"launches": sum(v[0] for v in rec.values()),
                   "top_ms": {q: round(v[1], 3) for q, v in sorted(rec.items(), key=lambda kv: -kv[1][1])[:8]}}
    nat.prof_enable(False)
    med = {k: statistics.median(v) for k, v in times.items()}
    out = {"workload": f"training step ({'mixed' if mixed else 'dirichlet'} family), {R} replicas, each a union batch of {B} hexagon meshes "
                       f"(n={n}): {batches[0].num_nodes} nodes per replica; fw_tol 1e-5 / bw_tol 1e-8, thresholds 500, jac_weight {jw}",
           "replicas": R, "bw_solver": bw_solver, "bw_gmres_lockstep": gmres_lockstep, "steps": steps, "s_per_step_median": med, "s_per_step_all": times, "one_more_step_profiled": kern}
    if only is None:
        out.update(lockstep_over_sequential=med["lockstep"] / med["sequential"],
                   lockstep_over_sequential_lin=med["lockstep"] / med["sequential_lin"])
    if lock is not None:
        dq = lock.net.deqdss
        out.update(lockstep_fw_nstep=[o["nstep"] for o in dq.last_forward], lockstep_bw_n_iter=[o.get("n_iter", o["nstep"]) for o in dq.last_backward])
    if seq:
        out["sequential_bw_n_iter"] = [t.net.deqdss.last_backward.get("n_iter", t.net.deqdss.last_backward["nstep"]) for t in seq]
    if seq_lin:
        out["sequential_lin_bw_n_iter"] = [t.net.deqdss.last_backward.get("n_iter", t.net.deqdss.last_backward["nstep"]) for t in seq_lin]
    print(json.dumps(out))


def main():
    rs = [a for a in sys.argv if a.startswith("replicas=")]
    if rs:
        ro = [a.split("=", 1)[1] for a in sys.argv if a.startswith("route=")]
        opt = {a.split("=", 1)[0]: a.split("=", 1)[1] for a in sys.argv if a.startswith(("bw_solver=", "lockstep="))}
        return replicas_main([a for a in sys.argv if not a.startswith(("replicas=", "route=", "bw_solver=", "lockstep="))],
                             int(rs[0].split("=", 1)[1]), ro[0] if ro else None, bw_solver=opt.get("bw_solver"),
                             gmres_lockstep=opt.get("lockstep", "0") not in ("0", ""))
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 13
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    cpu = int(sys.argv[4]) if len(sys.argv) > 4 else 1
    jw = float(sys.argv[5]) if len(sys.argv) > 5 else 0.0
    mixed = len(sys.argv) > 6 and sys.argv[6] == "mixed"
    data, nat = pkg("data"), pkg("_native")
    import numpy as np
    w = np.load(os.path.join(ROOT, "tests", "golden", "weights_mixed.npz" if mixed else "weights_dirichlet.npz"))
    sd = {k: torch.from_numpy(w[k]) for k in w.files}
    meshes = [data.make_hex_problem(n, seed=s, phase=0.37 * s, mixed=mixed) for s in range(B)]
    batch = data.collate(meshes)
    dev = torch.device("cuda:0")
    solver = pkg("utilities.solver")
    cfg = dict(latent_dim=10, n_layers=1, solver=solver.broyden, fw_tol=1e-5, fw_thres=500, bw_tol=1e-8, bw_thres=500)
    net = (pkg("mixed") if mixed else pkg("model_psignn")).ModelDEQDSS(cfg)
    net.load_state_dict(sd)
    net = net.to(dev).train()
    TrainModel = pkg("training_class").TrainModel
    tr = TrainModel(dict(loader_train=[], loader_val=[], model=net, config_model=net.config, lr_deq=1e-6, lr_ae=1e-6,
                         sched_step_deq=0.5, sched_step_ae=0.5, path_ckpt=None, min_loss_save=1e9, max_epochs=0,
                         gradient_clip=1e-2, sup_weight=0.0, jac_weight=jw))
    bd = batch.to(dev)
    warm, _ = tr.train_step(bd)  # warm-up (plan build, allocations); lr = 1e-6 keeps the weights at the checkpoint
    warm = float(warm.detach())
    torch.cuda.synchronize()
    nat.prof_enable(True)
    t0 = time.perf_counter()
    fw, bw, losses = [], [], []
    for _ in range(steps):
        loss, _ = tr.train_step(bd)
        fw.append(net.deqdss.last_forward["nstep"])
        bw.append(net.deqdss.last_backward["nstep"])
        losses.append(float(loss.detach()))
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    kern = nat.prof_collect()
    nat.prof_enable(False)
    out = {"workload": f"training step ({'mixed' if mixed else 'dirichlet'} family), union batch of {B} hexagon meshes (n={n}): {batch.num_nodes} nodes, "
                       f"{batch.num_edges} edges; fw_tol 1e-5 / bw_tol 1e-8, thresholds 500 (reference defaults), jac_weight {jw}",
           "gpu_s_per_step": dt, "gpu_graphs_per_s": B / dt, "first_step_loss": warm, "fw_nstep": fw, "bw_nstep": bw, "loss": losses,
           "kernels_ms_per_step": {k: round(v[1] / steps, 3) for k, v in sorted(kern.items(), key=lambda kv: -kv[1][1])[:12]}}
    if cpu:
        from oracle import psignn_oracle as orc
        torch.set_num_threads(min(32, os.cpu_count() or 1))
        t0 = time.perf_counter()
        probe = torch.randn(batch.num_nodes, 10, generator=torch.Generator().manual_seed(0)) if jw else None
        wl, _, _, ofw, obw = orc.training_step(sd, batch, fw_tol=1e-5, fw_thres=500, bw_tol=1e-8, bw_thres=500,
                                               jac_weight=jw, probe=probe)
        ct = time.perf_counter() - t0
        out.update(cpu_s_per_step=ct, cpu_threads=torch.get_num_threads(), cpu_fw_nstep=ofw["nstep"],
                   cpu_bw_nstep=obw["nstep"], cpu_loss=float(wl), speedup=ct / dt,
                   cpu_kind="port: oracle training_step (autograd on the restated f + restated broyden), first step only")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
