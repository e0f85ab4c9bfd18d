"""CRC-32 of the result and the ``rel_trace`` of the device solvers on fixed seeds: one JSON line.

The solver kernels use no atomics and fixed summation orders, so two builds of the library that run the same schedule on
the same statements give the same line; a differing CRC is a changed launch shape or statement, not noise.  Cases: three
rows of tests/golden/broyden_schedule.json through the host-driven Broyden solve (scripts/record_broyden_schedule.py), the
fused ``psignn_broyden_solve`` on a hex mesh, a ``psignn_broyden_solve_batch`` shard of three meshes, a stepwise Anderson solve
(beta = 0.5, m = 3), the lockstep Anderson solve of the same meshes, and a Picard solve.
    python scripts/broyden_bits.py [--out file.json]"""
import argparse
import json
import os
import struct
import sys
import zlib

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import record_broyden_schedule as rec   # noqa: E402
from record_broyden_schedule import ROOT, pkg   # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
TABLE_CASES = ("m4090", "width_switch", "above_reg_fold")


def crcs(out):
    """result and rel_trace of a solver's output dict, as 'crc(result),crc(rel_trace as float64)'."""
    res = zlib.crc32(out["result"].detach().contiguous().cpu().numpy().tobytes())
    tr = zlib.crc32(b"".join(struct.pack("<d", float(v)) for v in out["rel_trace"]))
    return f"{res:08x},{tr:08x}"


def mesh_maps(dev, sizes):
    data, eng = pkg("data"), pkg("engine")
    from oracle import psignn_oracle as orc
    w = np.load(os.path.join(GOLDEN, "weights_dirichlet.npz"))
    sd = {k: torch.from_numpy(w[k]) for k in w.files}
    weights = eng.PackedWeights(sd, dev)
    fms = []
    for s, n in enumerate(sizes):
        mesh = data.make_hex_problem(n, seed=s, compute_sol=False, phase=0.37 * s)
        md = mesh.to(dev)
        with torch.no_grad():
            h0 = orc.encoder(sd, mesh.x)
        fms.append(eng.FixedPointMap(eng.MeshPlan(md), weights, h0.to(dev), md.prb_data, None))
    return fms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "broyden_bits.py needs a GPU"
    dev = torch.device("cuda:0")
    eng, solver = pkg("engine"), pkg("utilities.solver")
    res = {"device": torch.cuda.get_device_name(0), "crc": "crc32 of the result bytes,crc32 of rel_trace as float64"}
    by_name = {c["case"]: c for c in rec.cases()}
    for name in TABLE_CASES:
        res[name] = crcs(rec.run_case(by_name[name], dev)[1])
    fms = mesh_maps(dev, (26, 34, 30))
    fm = fms[1]
    res["broyden_solve hex34"] = crcs(solver.broyden(fm, fm.h0, threshold=40, eps=0.0, keep_trace=False))
    total = sum(f.plan.N for f in fms) * 10
    svs = [eng.DeviceBroyden(plan=f.plan, threshold=40, keep_trace=False, shard_elems=total) for f in fms]
    for i, o in enumerate(eng.broyden_solve_batch(svs, fms, 0.0)):
        res[f"broyden_solve_batch mesh{i}"] = crcs(o)
    for sv in svs:
        sv.close()
    res["anderson hex34 beta0.5 m3"] = crcs(solver.anderson(fm, fm.h0, m=3, beta=0.5, threshold=30, eps=0.0))
    for i, o in enumerate(solver.anderson_batch(fms, m=3, beta=0.5, threshold=30, eps=0.0)):
        res[f"anderson_batch mesh{i}"] = crcs(o)
    res["picard hex34"] = crcs(solver.forward_iteration(fm, fm.h0, eps=0.0, threshold=30))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
