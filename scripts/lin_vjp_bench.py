"""Transposed product of the stored linearisation against the tiled VJP: one JSON line.

Median HIP-event times of fmap.vjp_p (k_vjp_tile_a + k_vjp_tile_b), lin.vjp_p (k_vjp_lin), lin.jvp_p (k_jvp_lin) and one
lin.build at the 1M-node bench mesh and at 100k nodes; then one implicit_backward (the hex13 fixture, a 50-graph union batch) with
and without the model's ``bw_linearize``, with its steps and final residual.
    python scripts/lin_vjp_bench.py [--reps 30] [--out file.json] [--products-only]   (--products-only: the 1M-node products alone,
    e.g. under rocprofv3 --kernel-trace --stats)

--family mixed: the mixed checkpoint (tests/golden/weights_mixed.npz) on make_hex_problem(182 / 440, mixed=True) (99 919 / 582 121
nodes): build, jvp_p and vjp_p of a Linearization that stores the Neumann rows (neumann="stored") against the "direct" handle in
the same process, the two alternating call by call; one implicit_backward (hex13 mixed, a 50-graph mixed union batch) with
lin_neumann "direct" and "stored"; with --parity FILE also the float64 parity of both handles per row class at 547, 10 981, 99 919
and 582 121 nodes (CPU oracle).  --products-only: the 582 121-node products alone."""
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


def weights(kind="dirichlet"):
    w = np.load(os.path.join(ROOT, "tests", "golden", f"weights_{kind}.npz"))
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


# ---------------------------------------------------------------------------------------------------------------- mixed family
def _mixed_map(n, seed, sd):
    mesh = pkg.data.make_hex_problem(n, seed=seed, mixed=True, compute_sol=False)
    md = mesh.to(dev)
    net = importlib.import_module("psi-gnn_amd.mixed").ModelPSIGNN(dict(latent_dim=10, n_layers=1))
    net.load_state_dict(sd)
    net = net.to(dev).eval()
    with torch.no_grad():
        h0 = net.autoencoder.encoder(md.x)
    return mesh, net.deqdss.f.bind(h0, md)


def timed_pair(fa, fb, reps):
    """Medians (us) of two calls timed alternately, a b a b ..., after one warm call of each."""
    fa(), fb()
    ta, tb = [], []
    for _ in range(reps):
        for fn, ts in ((fa, ta), (fb, tb)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(ta)), float(np.median(tb))


def products_mixed(n, seed, sd, reps):
    mesh, fm = _mixed_map(n, seed, sd)
    Hp = fm.to_plan(fm.h0)
    for _ in range(6):
        Hp = fm.fp(Hp)
    st, di = eng.Linearization(fm, neumann="stored").build(Hp), eng.Linearization(fm, neumann="direct").build(Hp)
    gen = torch.Generator(device=dev).manual_seed(1)
    Wp, Vp = torch.randn(Hp.shape, device=dev, generator=gen), torch.randn(Hp.shape, device=dev, generator=gen)
    out = torch.empty_like(Wp)
    r = {"N": int(fm.plan.N), "Ep": int(fm.plan.Ep), "tiles": int(fm.plan.n_tiles)}
    for key, fs, fd in (("vjp_p", lambda: st.vjp_p(Wp, out=out), lambda: di.vjp_p(Wp, out=out)),
                        ("jvp_p", lambda: st.jvp_p(Wp, out=out), lambda: di.jvp_p(Wp, out=out)),
                        ("build", lambda: st.build(Hp), lambda: di.build(Hp))):
        a, b = timed_pair(fs, fd, reps)
        r[key] = {"stored_us": a, "direct_us": b, "ratio": a / b}
    r["fmap_vjp_p_us"] = timed(lambda: fm.vjp_p(Hp, Wp), reps)
    r["fmap_jvp_p_us"] = timed(lambda: fm.jvp_p(Hp, Wp), reps)
    r["lin_bytes"] = {"stored": int(eng.nat.lib().psignn_lin_bytes(st.handle)), "direct": int(eng.nat.lib().psignn_lin_bytes(di.handle))}
    for name, lin in (("stored", st), ("direct", di)):
        jv = lin.jvp_p(Vp).double()
        r["adjoint_gap_" + name] = abs(float((Wp.double() * jv).sum()) - float((lin.vjp_p(Wp).double() * Vp.double()).sum())) / (
            float(Wp.double().norm()) * float(jv.norm()))
    r["rel_l2_stored_vs_fmap"] = {"vjp_p": float((st.vjp_p(Wp) - fm.vjp_p(Hp, Wp)).norm() / fm.vjp_p(Hp, Wp).norm()),
                                  "jvp_p": float((st.jvp_p(Wp) - fm.jvp_p(Hp, Wp)).norm() / fm.jvp_p(Hp, Wp).norm())}
    st.close(), di.close()
    return r


def backward_mixed(mesh, sd, label):
    mixed = importlib.import_module("psi-gnn_amd.mixed")
    mesh = mesh.to(dev)
    rows, h_star = {}, None
    for key, kw in (("default", {}), ("direct", dict(bw_linearize=True, lin_neumann="direct")),
                    ("stored", dict(bw_linearize=True, lin_neumann="stored"))):
        net = mixed.ModelDEQDSS(dict(latent_dim=10, n_layers=1, fw_tol=1e-7, fw_thres=600, **kw))
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
        rows[key] = {"ms": e0.elapsed_time(e1), "nstep": o["nstep"], "n_iter": o["n_iter"], "lowest": o["lowest"], "result": o["result"]}
    base = rows["default"].pop("result")
    for key in ("direct", "stored"):
        rows[key]["rel_l2_vs_default"] = float((rows[key].pop("result") - base).norm() / base.norm())
    return {"mesh": label, "N": int(mesh.num_nodes), "bw_tol": 1e-8, "bw_thres": 300, **rows}


def parity_mixed(n, seed, sd):
    """rel-L2 against the float64 CPU oracle of both handles, all rows and per row class, at f(f(h0)) and two steps on."""
    from oracle import psignn_oracle as orc
    mesh, fm = _mixed_map(n, seed, sd)
    s64 = {k: v.double() for k, v in sd.items()}
    m64 = mesh.clone()
    for k, v in list(vars(mesh).items()):
        if torch.is_tensor(v) and v.is_floating_point():
            setattr(m64, k, v.double())
    fl = fm.plan.export("node_flags").astype(np.int64)
    neu = (fl & 3) == 2
    src, dst = mesh.edge_index[0].numpy(), mesh.edge_index[1].numpy()
    near = np.zeros(len(fl), bool)
    near[src[neu[dst]]] = True
    near[dst[neu[src]]] = True
    sel = {"all": np.ones(len(fl), bool), "neumann": neu, "near": near & ~neu, "rest": ~near & ~neu}
    st = eng.Linearization(fm, neumann="stored")
    Hp = fm.fp(fm.fp(fm.to_plan(fm.h0)))
    rows = []
    for i in range(2):
        st.build(Hp)
        v = torch.randn(len(fl), 10, generator=torch.Generator().manual_seed(30 + i))
        Vp = fm.to_plan(v.to(dev))
        h = fm.from_plan(Hp).cpu().double()
        h0 = fm.h0.cpu().double()
        with torch.no_grad():
            want = {"jvp": orc.function_jvp(s64, h, h0, m64, v.double())}
        want["vjp"] = orc.function_vjp(s64, h, h0, m64, v.double())
        got = {"jvp": (st.jvp_p(Vp), fm.jvp_p(Hp, Vp)), "vjp": (st.vjp_p(Vp), fm.vjp_p(Hp, Vp))}
        for prod in ("jvp", "vjp"):
            for cls, m in sel.items():
                mm = torch.from_numpy(m)
                e = [float((fm.from_plan(g).cpu().double()[mm] - want[prod][mm]).norm() / want[prod][mm].norm()) for g in got[prod]]
                rows.append({"state": i, "product": prod, "rows": cls, "n_rows": int(m.sum()), "e_stored": e[0], "e_direct": e[1]})
        Hp = fm.fp(fm.fp(Hp))
    st.close()
    return {"N": int(fm.plan.N), "neumann_rows": int(neu.sum()), "errors": rows}


def main_mixed(a):
    sd = weights("mixed")
    res = {"device": torch.cuda.get_device_name(0), "family": "mixed",
           "timing": "median of HIP-event pairs around one call, stored and direct handle alternating, after one warm call"}
    res["mesh582k"] = products_mixed(440, 2, sd, a.reps)
    if not a.products_only:
        res["mesh100k"] = products_mixed(182, 0, sd, a.reps)
        res["implicit_backward_hex13"] = backward_mixed(pkg.data.make_hex_problem(13, seed=1, mixed=True), sd, "hex13 mixed")
        union = pkg.data.collate([pkg.data.make_hex_problem(13, seed=s, mixed=True) for s in range(50)])
        res["implicit_backward_union50"] = backward_mixed(union, sd, "50 x hex13 mixed union batch")
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if a.parity:
        par = {"reference": "oracle.psignn_oracle.function_jvp / function_vjp in float64 on the CPU",
               "hex13": parity_mixed(13, 1, sd), "hex60": parity_mixed(60, 3, sd), "hex182": parity_mixed(182, 0, sd),
               "hex440": parity_mixed(440, 2, sd)}
        with open(a.parity, "w") as f:
            f.write(json.dumps(par) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--products-only", action="store_true")
    ap.add_argument("--family", choices=("dirichlet", "mixed"), default="dirichlet")
    ap.add_argument("--parity", default=None, help="mixed family: write the float64 parity per row class to this file")
    a = ap.parse_args()
    if a.family == "mixed":
        return main_mixed(a)
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
