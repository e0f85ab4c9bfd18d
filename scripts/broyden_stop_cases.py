"""Which natural Broyden solves meet the stagnation rule or the protective break: profiles/broyden_stop_cases.json.

Every natural solve of tests/test_gpu_broyden_stop.py (parts b and c: fused forward, the two adjoint solves, float64 forward and
adjoint, the ragged shard forward and adjoint) runs once on the GPU to threshold 300 with eps = 0 -- no tolerance and no stagnation
stop, so the trace is the whole trajectory unless the protective break ends it (the iterates do not depend on eps).  The trace is then
replayed on the CPU (tests/broyden_stop_ref.replay) over a scan of eps, 8 values per decade: per solver, the eps range over which the
reference's rules end the solve on stagnation (reason 2), the value chosen for the test (the median of that range) and whether any
break (reason 3) occurs.

    python scripts/broyden_stop_cases.py                    # measure on cuda:0, scan, write the profile
    python scripts/broyden_stop_cases.py --traces T.json    # scan traces measured earlier (no GPU needed)
    python scripts/broyden_stop_cases.py --dump T.json      # also keep the full traces
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
KEYS = ("n_iter", "nstep", "stop_reason", "prot_break", "lowest", "rel_trace", "abs_trace")
THRESHOLD = 300


def measure():
    import torch

    import test_gpu_broyden_stop as T
    dev = torch.device("cuda:0")
    res = {}
    for label, make in T.natural(dev).items():
        o, _ = make().run(0.0, THRESHOLD, False)
        res[label] = {k: o[k] for k in KEYS}
    sh = T.Shard(dev)
    for adj in (False, True):
        for mode in ("rel", "abs"):
            outs, _ = sh.run(adj, 0.0, THRESHOLD, mode)
            for i, o in enumerate(outs):
                res[f"shard_{'adjoint' if adj else 'forward'}/{i}/{mode}"] = {k: o[k] for k in KEYS}
    return res


def scan(res):
    from broyden_stop_ref import replay
    grid = [10.0 ** (e / 8.0) for e in range(-17 * 8, 3 * 8 + 1)]
    out = {}
    for label, o in res.items():
        mode = label.rsplit("/", 1)[1]
        n = o["n_iter"]
        tr = np.array(o[mode + "_trace"][:n])
        hits = []
        for eps in grid:
            rp = replay(o["rel_trace"], o["abs_trace"], n, eps, THRESHOLD, 10, mode)
            if rp["stop_reason"] == 2:
                hits.append((eps, rp["n_iter"], rp["nstep"]))
        row = {"steps_run": n, "ended_on": o["stop_reason"], "lowest": o["lowest"], "lowest_step": o["nstep"],
               "first": float(tr[0]), "last": float(tr[-1]), "max": float(tr.max()),
               "tail30_max_over_min": float(tr[-30:].max() / tr[-30:].min()),
               "natural_break": bool(o["prot_break"])}
        if hits:
            eps, step, low = hits[len(hits) // 2]
            row["stagnation"] = {"eps_from": hits[0][0], "eps_to": hits[-1][0], "chosen_eps": float(f"{eps:.3e}"), "stops_at": step,
                                 "lowest_step": low}
            rp = replay(o["rel_trace"], o["abs_trace"], n, row["stagnation"]["chosen_eps"], THRESHOLD, 10, mode)
            assert (rp["stop_reason"], rp["n_iter"]) == (2, step), (label, rp["stop_reason"], rp["n_iter"], step)
        else:
            row["stagnation"] = None
        out[label] = row
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--traces")
    ap.add_argument("--dump")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "broyden_stop_cases.json"))
    a = ap.parse_args()
    res = json.load(open(a.traces)) if a.traces else measure()
    if a.dump:
        json.dump(res, open(a.dump, "w"))
    rows = scan(res)
    none = sorted(k for k, r in rows.items() if r["stagnation"] is None)
    doc = {"what": "natural Broyden solves on the MI355X, threshold 300, eps 0; the trace replayed over eps = 10^(k/8), k = -136 .. 24 "
                   "(tests/broyden_stop_ref.replay, seq_len 10)",
           "no_natural_stagnation": none,
           "natural_protective_break": sorted(k for k, r in rows.items() if r["natural_break"]),
           "solves": rows}
    json.dump(doc, open(a.out, "w"), indent=1)
    for k, r in rows.items():
        s = r["stagnation"]
        print(f"{k}: lowest {r['lowest']:.3e} at {r['lowest_step']}, tail ratio {r['tail30_max_over_min']:.2f}, "
              + (f"stagnation for eps {s['eps_from']:.2e} .. {s['eps_to']:.2e}: chosen {s['chosen_eps']:.3e} -> step {s['stops_at']}, lowest at {s['lowest_step']}"
                 if s else "no eps gives a stagnation stop"))


if __name__ == "__main__":
    main()
