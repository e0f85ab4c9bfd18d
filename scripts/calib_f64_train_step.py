"""Where the gates of tests/test_gpu_f64_train_step.py and tests/test_host_f64_train_step.py come from.  The rule is that of
tests/test_gpu_f64_pgrad.py: a gate is 250 x the float64 CPU oracle's own spread when its summation order changes -- the only freedom
a correct float64 statement has.  CPU only, on exactly the cases of the tests (tests/train_step_ref.py):

1. the residual ``A u - y`` and ``A^T w`` in the oracle's index_add_ form, edge list permuted and nodes renumbered, three seeds each,
   and the defect the oracle itself leaves in ``<w, A u> = <A^T w, u>``;
2. ``torch.mean((a - b) ** 2)`` with its elements permuted, on the lengths of the test;
3. ``train_step_ref`` at the oracle step's own ``h*`` and ``y`` against ``orc.training_step`` (the same graph), then with the edge
   list permuted and the nodes renumbered, three seeds each: per class (matrices of f, vectors / scalars of f, the autoencoder's
   tensors, ``grad_h``, loss scalars) the worst relative L2;
4. on the fixtures, the distance between the oracle step at tolerances 1e-11 and 1e-10: the solver's own share, per class.

    python scripts/calib_f64_train_step.py
"""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import train_step_ref as ts   # noqa: E402

SEEDS = (1, 2, 3)
MSE_CHUNK = 1024
MSE_LENGTHS = [1, MSE_CHUNK - 1, MSE_CHUNK, MSE_CHUNK + 1, 256 * MSE_CHUNK + 1, 109810]


def residual_spread():
    tot = {"r": 0.0, "t": 0.0, "dual": 0.0}
    for name in ts.RESIDUAL_NAMES:
        mesh, _, u, w = ts.residual_case(name)
        ei, a, y = mesh.edge_index, mesh.a_ij.double(), mesh.y.double()
        r0, t0 = ts.residual_ref(ei, a, u, y), ts.residual_t_ref(ei, a, w)
        Au = r0 + y
        dual = abs(float((w * Au).sum()) - float((t0 * u).sum())) / (float(w.norm()) * float(Au.norm()))
        worst = {"r": 0.0, "t": 0.0}
        if ei.shape[1] != mesh.num_nodes:
            for nodes in (False, True):
                for seed in SEEDS:
                    mp, (up, wp), inv = ts.permuted(mesh, [u, w], seed, nodes)
                    r = ts.residual_ref(mp.edge_index, mp.a_ij.double(), up, mp.y.double())
                    t = ts.residual_t_ref(mp.edge_index, mp.a_ij.double(), wp)
                    if inv is not None:
                        r, t = r[inv], t[inv]
                    worst["r"] = max(worst["r"], ts.rel(r, r0))
                    worst["t"] = max(worst["t"], ts.rel(t, t0))
        print(f"residual {name:28s} A u - y {worst['r']:.1e}  A^T w {worst['t']:.1e}  duality defect {dual:.1e}", flush=True)
        tot = {"r": max(tot["r"], worst["r"]), "t": max(tot["t"], worst["t"]), "dual": max(tot["dual"], dual)}
    print("residual worst: " + "  ".join(f"{k} {v:.1e}" for k, v in tot.items()), flush=True)


def mse_spread():
    worst = 0.0
    for n in MSE_LENGTHS:
        gen = torch.Generator().manual_seed(70 + n % 97)
        a, b = torch.randn(n, generator=gen, dtype=torch.float64), torch.randn(n, generator=gen, dtype=torch.float64)
        base = float(torch.mean((a - b) ** 2))
        w = 0.0
        for seed in SEEDS:
            p = torch.randperm(n, generator=torch.Generator().manual_seed(seed))
            w = max(w, abs(float(torch.mean((a[p] - b[p]) ** 2)) - base) / base)
            w = max(w, abs(float(((a[p] - b[p]) ** 2).cumsum(0)[-1]) / n - base) / base)   # one sequential order as well
        print(f"mse n = {n:7d}: spread of the mean {w:.1e}", flush=True)
        worst = max(worst, w)
    print(f"mse worst: {worst:.1e}", flush=True)


def _classes(grads, base, worst):
    for k, t in base.items():
        if not bool(t.any()):
            assert not bool(grads[k].any()), k
            continue
        c = ts.tensor_class(k, t)
        r = ts.rel(grads[k], t)
        if r > worst[c][0]:
            worst[c] = (r, k)


def step_spread():
    tot = {}
    for name in ts.STEP_NAMES:
        t0 = time.time()
        o = ts.oracle_at(name)
        sd, mesh, probe = o["sd"], o["mesh"], o["probe"]
        hs, y = o["fw"]["result"].detach(), o["bw"]["result"].detach()
        print(f"step {name}: oracle step {time.time() - t0:.1f} s, fw nstep {o['fw']['nstep']} lowest {o['fw']['lowest']:.2e}, "
              f"bw nstep {o['bw']['nstep']} lowest {o['bw']['lowest']:.2e}", flush=True)
        loss, dic, grads, grad_h = ts.train_step_ref(sd, mesh, hs, y, probe, 1.0)
        same = max(ts.rel(grads[k], o["grads"][k]) for k in grads)
        same_l = max(abs(float(dic[k]) - float(o["loss_dic"][k])) for k in dic)
        print(f"step {name}: train_step_ref against orc.training_step: worst tensor {same:.1e}, worst loss term {same_l:.1e}, "
              f"loss {abs(float(loss) - float(o['loss'])):.1e}", flush=True)
        worst = {"matrix": (0.0, ""), "vector": (0.0, ""), "mlp": (0.0, ""), "grad_h": (0.0, ""), "loss": (0.0, "")}
        for nodes in (False, True):
            for seed in SEEDS:
                mp, (hp, yp, pp), inv = ts.permuted(mesh, [hs, y, probe], seed, nodes)
                l2, d2, g2, gh2 = ts.train_step_ref(sd, mp, hp, yp, pp, 1.0)
                _classes(g2, grads, worst)
                r = ts.rel(gh2 if inv is None else gh2[inv], grad_h)
                if r > worst["grad_h"][0]:
                    worst["grad_h"] = (r, "grad_h")
                for k in list(dic) + ["loss"]:
                    a, b = (float(l2), float(loss)) if k == "loss" else (float(d2[k]), float(dic[k]))
                    r = abs(a - b) / abs(b) if b != 0 else abs(a - b)
                    if r > worst["loss"][0]:
                        worst["loss"] = (r, k)
        print(f"step {name}: spread " + "  ".join(f"{c} {v[0]:.1e} ({v[1]})" for c, v in worst.items()), flush=True)
        for c, v in worst.items():
            tot[c] = max(tot.get(c, 0.0), v[0])
    print("step worst: " + "  ".join(f"{c} {v:.1e}" for c, v in tot.items()), flush=True)


def tolerance_distance():
    tot = {}
    for name in ts.FIXTURES:
        o = ts.oracle_at(name)
        t0 = time.time()
        loss, dic, grads, fw, bw = ts.oracle_step(o["sd"], o["mesh"], o["probe"], (1e-10, 1000), (1e-10, 800))
        worst = {"matrix": (0.0, ""), "vector": (0.0, ""), "mlp": (0.0, ""), "loss": (0.0, "")}
        _classes(grads, o["grads"], worst)
        for k in dic:
            a, b = float(dic[k]), float(o["loss_dic"][k])
            r = abs(a - b) / abs(b) if b != 0 else abs(a - b)
            if r > worst["loss"][0]:
                worst["loss"] = (r, k)
        dh = ts.rel(fw["result"], o["fw"]["result"])
        dy = ts.rel(bw["result"], o["bw"]["result"])
        print(f"tolerance {name} ({time.time() - t0:.1f} s): 1e-10 against 1e-11: h* {dh:.1e}  y {dy:.1e}  "
              + "  ".join(f"{c} {v[0]:.1e} ({v[1]})" for c, v in worst.items()), flush=True)
        for c, v in worst.items():
            tot[c] = max(tot.get(c, 0.0), v[0])
        tot["h_star"], tot["y"] = max(tot.get("h_star", 0.0), dh), max(tot.get("y", 0.0), dy)
    print("tolerance worst: " + "  ".join(f"{c} {v:.1e}" for c, v in tot.items()), flush=True)


if __name__ == "__main__":
    residual_spread()
    mse_spread()
    step_spread()
    tolerance_distance()
