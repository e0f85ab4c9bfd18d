"""Transposed product of the stored linearisation against the tiled VJP: one JSON line.

Median HIP-event times of fmap.vjp_p (k_vjp_tile_a + k_vjp_tile_b), lin.vjp_p (k_vjp_lin), lin.jvp_p (k_jvp_lin) and one
lin.build at the 1M-node bench mesh and at 100k nodes; then one implicit_backward (the hex13 fixture, a 50-graph union batch) with
and without the model's ``bw_linearize``, with its steps and final residual.
    python scripts/lin_vjp_bench.py [--reps 30] [--out file.json] [--products-only]   (--products-only: the 1M-node products alone,
    e.g. under rocprofv3 --kernel-trace --stats)"""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("psi-gnn_amd")
eng = importlib.import_module("psi-gnn_amd.engine")
mp = importlib.import_module("psi-gnn_amd.model_psignn")
dev = torch.device("cuda:0")


def weights():
    w = np.load(os.path.join(ROOT, "tests", "golden", "weights_dirichlet.npz"))
    return {k: torch.from_numpy(w[k]) for k in w.files}


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(ts))


def products(nodes, sd, reps):
    n = pkg.data.hex_n_for_nodes(nodes)
    mesh = pkg.data.make_hex_problem(n, seed=0, compute_sol=False).to(dev)
    net = mp.ModelPSIGNN(dict(latent_dim=10, n_layers=1))
    net.load_state_dict(sd)
    net = net.to(dev).eval()
    with torch.no_grad():
        h0 = net.autoencoder.encoder(mesh.x)
    fm = net.deqdss.f.bind(h0, mesh)
    Hp = fm.to_plan(fm.h0)
    for _ in range(20):   # a state along the forward iteration, not the encoder output
        Hp = fm.fp(Hp)
    lin = fm.linearize_p(Hp)
    Wp = torch.randn(Hp.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    out = torch.empty_like(Wp)
    r = {"N": int(fm.plan.N), "Ep": int(fm.plan.Ep), "lin_bytes_before_vjp": int(eng.nat.lib().psignn_lin_bytes(lin.handle))}
    r["fmap_vjp_p_us"] = timed(lambda: fm.vjp_p(Hp, Wp), reps)
    r["lin_vjp_p_us"] = timed(lambda: lin.vjp_p(Wp, out=out), reps)
    r["lin_jvp_p_us"] = timed(lambda: lin.jvp_p(Wp, out=out), reps)
    r["lin_build_us"] = timed(lambda: lin.build(Hp), reps)
    # first transposed product after a build (fills the transposed masks)
    r["lin_vjp_p_first_after_build_us"] = timed(lambda: (lin.build(Hp), lin.vjp_p(Wp, out=out)), reps) - r["lin_build_us"]
    r["ratio_lin_vjp_to_vjp_p"] = r["lin_vjp_p_us"] / r["fmap_vjp_p_us"]
    r["lin_bytes"] = int(eng.nat.lib().psignn_lin_bytes(lin.handle))
    Vp = torch.randn(Hp.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(2))
    jv = lin.jvp_p(Vp).double()
    r["adjoint_gap"] = abs(float((Wp.double() * jv).sum()) - float((lin.vjp_p(Wp).double() * Vp.double()).sum())) / (
        float(Wp.double().norm()) * float(jv.norm()))
    r["rel_l2_lin_vjp_vs_vjp_p"] = float((lin.vjp_p(Wp) - fm.vjp_p(Hp, Wp)).norm() / fm.vjp_p(Hp, Wp).norm())
    lin.close()
    return r


def backward(mesh, sd, label):
    mesh = mesh.to(dev)
    rows = {}
    h_star = None
    for opt in (False, True):
        net = mp.ModelDEQDSS(dict(latent_dim=10, n_layers=1, fw_tol=1e-7, fw_thres=600, bw_linearize=opt))
        net.load_state_dict(sd)
        net = net.to(dev).eval()
        with torch.no_grad():
            h0 = net.autoencoder.encoder(mesh.x)
            if h_star is None:
                h_star = net.deqdss(h0, mesh)["result"]
            grad = torch.randn(h_star.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(3))
            net.deqdss.implicit_backward(h_star, h0, mesh, grad)   # buffers
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            o = net.deqdss.implicit_backward(h_star, h0, mesh, grad)
            e1.record()
            e1.synchronize()
        rows["linearized" if opt else "default"] = {"ms": e0.elapsed_time(e1), "nstep": o["nstep"], "n_iter": o["n_iter"],
                                                    "lowest": o["lowest"], "result": o["result"]}
    d, l = rows["default"], rows["linearized"]
    rd = d.pop("result")
    rel = float((l.pop("result") - rd).norm() / rd.norm())
    return {"mesh": label, "N": int(mesh.num_nodes), "bw_tol": 1e-8, "bw_thres": 300, "default": d, "linearized": l,
            "speedup": d["ms"] / l["ms"], "rel_l2_linearized_vs_default": rel}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--products-only", action="store_true")
    a = ap.parse_args()
    sd = weights()
    res = {"device": torch.cuda.get_device_name(0), "timing": "median of HIP-event pairs around one call, after one warm call"}
    res["mesh1m"] = products(1_000_000, sd, a.reps)
    if a.products_only:
        print(json.dumps(res))
        return
    res["mesh100k"] = products(100_000, sd, a.reps)
    hex13 = pkg.data.make_hex_problem(13, seed=0)
    res["implicit_backward_hex13"] = backward(hex13, sd, "hex13")
    union = pkg.data.collate([pkg.data.make_hex_problem(13, seed=s) for s in range(50)])
    res["implicit_backward_union50"] = backward(union, sd, "50 x hex13 union batch")
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
