"""CRC-32 of the raw output bytes of every plan-order entry point that runs a tile kernel, on fixed seeds: one JSON line.

The tile kernels use no atomics and fixed summation orders, so two builds of the library that compute the same statements
give the same line; a differing CRC is a changed statement, not noise.  Entry points: FixedPointMap.fp, jvp_p, vjp_p,
param_vjp_p and vjp_backward_p (the last two: dirichlet family; the mixed family's record kernels run under param_vjp),
dsgps_step_p, dsgps_step_backward, dss_step_p, and Linearization.jvp_p / vjp_p; on make_hex_problem(13) (547 nodes, three
tiles) and make_hex_problem(182) (about 100k nodes), both families.  Each call runs twice: "a,b" with a == b shows run-to-run
identity.
    python scripts/tile_bits.py [--out file.json]"""
import argparse
import importlib
import json
import os
import sys
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = lambda n="": importlib.import_module("psi-gnn_amd" + ("." + n if n else ""))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def weights(name, drop=()):
    w = np.load(os.path.join(GOLDEN, f"weights_{name}.npz"))
    return {k: torch.from_numpy(w[k]) for k in w.files if k not in drop}, w


def crc(out, c=0):
    """CRC-32 over the bytes of a tensor, or of the tensors of a tuple / list / dict (by sorted key) in order."""
    if torch.is_tensor(out):
        return zlib.crc32(out.detach().contiguous().cpu().numpy().tobytes(), c)
    for t in ([out[k] for k in sorted(out)] if isinstance(out, dict) else out):
        c = crc(t, c)
    return c


def twice(fn):
    a, b = crc(fn()), crc(fn())
    return f"{a:08x},{b:08x}"


def psignn(n, mixed, dev):
    data, eng = pkg("data"), pkg("engine")
    mesh = data.make_hex_problem(n, seed=0, mixed=mixed, compute_sol=False)
    md = mesh.to(dev)
    sd, _ = weights("mixed" if mixed else "dirichlet")
    N = mesh.num_nodes
    gen = torch.Generator().manual_seed(21)
    h0, h, v, wv, gb = (0.3 * torch.randn(N, 10, generator=gen) for _ in range(5))
    gb /= N
    nrm = getattr(md, "unit_normal_vector", None)
    plan = eng.MeshPlan(md)
    fm = eng.FixedPointMap(plan, eng.PackedWeights(sd, dev), h0.to(dev), md.prb_data, nrm)
    Hp, Vp, Wp, Gp = (fm.to_plan(t.to(dev)) for t in (h, v, wv, gb))
    r = {"N": int(plan.N), "tiles": int(plan.export("tile_ptr").shape[0] - 1)}
    r["fp"] = twice(lambda: fm.fp(Hp))
    r["jvp_p"] = twice(lambda: fm.jvp_p(Hp, Vp))
    r["vjp_p"] = twice(lambda: fm.vjp_p(Hp, Wp))
    if mixed:
        r["param_vjp"] = twice(lambda: fm.param_vjp(h.to(dev), wv.to(dev)))
    else:
        r["param_vjp_p"] = twice(lambda: fm.param_vjp_p(Hp, Wp))
        r["vjp_backward_p"] = twice(lambda: fm.vjp_backward_p(Hp, Wp, Gp))
    lin = fm.linearize_p(Hp)   # control: the stored linearisation's kernels
    r["lin.jvp_p"] = twice(lambda: lin.jvp_p(Vp))
    r["lin.vjp_p"] = twice(lambda: lin.vjp_p(Wp))
    lin.close()
    ds, _ = weights("dsgps_mixed" if mixed else "dsgps", drop=("k",))
    h0p, prbp, nrmp = fm._p
    wd = eng.pack_dsgps(ds, dev)
    r["dsgps_step_p"] = twice(lambda: eng.dsgps_step_p(plan, wd, Hp, h0p, prbp, nrmp))
    wf, wg = eng.pack_dsgps_train(ds, dev)

    def dsgps_bw():
        return eng.dsgps_step_backward(plan, wf, wg, h.to(dev), md.prb_data, wv.to(dev), nrm)
    r["dsgps_step_backward"] = twice(dsgps_bw)
    if not mixed:
        dss = pkg("dss")
        sdss, raw = weights("dss", drop=("k", "alpha"))
        mesh.sol = torch.zeros_like(mesh.x)
        b = dss.to_dss_batch(mesh).to(dev)
        dplan = dss.DeepStatisticalSolver._plan(b)
        wp = eng.pack_dss(sdss, int(raw["k"]), dev)
        hp, bp = dplan.permute(h.to(dev), True), dplan.permute(b.b_prime_norm, True)
        r["dss_step_p"] = twice(lambda: eng.dss_step_p(dplan, wp, 3, 1.0, hp, bp))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tile_bits.py needs a GPU"
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "crc": "crc32 of the output bytes, first call,second call"}
    for n in (13, 182):
        for mixed in (False, True):
            res[f"hex{n}_{'mixed' if mixed else 'dirichlet'}"] = psignn(n, mixed, dev)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
