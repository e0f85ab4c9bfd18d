"""The Broyden solver's schedule as the built library runs it: one row per case, tests/golden/broyden_schedule.json.

Each case creates one ``engine.DeviceBroyden`` (environment knobs set first: they are read when the handle is created) and
runs ``solve_callable`` on the linear map f(x) = c * x + b with eps = 0, so the solve makes exactly ``thr`` iterations.  A row
holds what ``broyden_shape`` / ``update_chain`` (csrc/solver_shapes.h) decide from the case's inputs alone:

    nbytes   ``psignn_broyden_bytes`` of the handle
    iters    per iteration, the update chain's launches in order as [kernel name, stated bytes / M]

Stated bytes are exact multiples of M (asserted).  tests/host/solver_shapes_check.cpp recomputes every row on the CPU from
the header; tests/test_gpu_solver_forms.py compares three rows with the library on the GPU.  Regenerate (only when a schedule
change is intended):
    python scripts/record_broyden_schedule.py --out tests/golden/broyden_schedule.json"""
import argparse
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = lambda n="": importlib.import_module("psi-gnn_amd" + ("." + n if n else ""))

KNOBS = ("PSIGNN_VEC16_MIN", "PSIGNN_JGROUPS", "PSIGNN_VEC_AX4", "PSIGNN_UVU", "PSIGNN_U2D_FORM", "PSIGNN_U2D_KMAX", "PSIGNN_U2D_KEEP")
# launches of update_chain (everything else in the log -- k_resid, k_xnext, k_begin -- belongs to its callers)
CHAIN = {"k_sweep_u1", "k_sweep_v", "k_sweep_u2", "k_sweep_u1_bf16", "k_sweep_v_bf16", "k_sweep_u2_bf16", "k_sweep_u2d", "k_reduce_check",
         "k_reduce_cb", "k_dots", "k_axpy", "k_axpy_combine", "k_final"}
ENVS = {   # tests/test_gpu_solver_forms.py::ENVS
    "default": {},
    "reg": {"PSIGNN_U2D_FORM": "reg"},
    "lds": {"PSIGNN_U2D_FORM": "lds"},
    "keep8": {"PSIGNN_U2D_FORM": "reg", "PSIGNN_U2D_KEEP": "8"},
    "window_from_5": {"PSIGNN_U2D_FORM": "reg", "PSIGNN_U2D_KMAX": "4", "PSIGNN_U2D_KEEP": "2"},
    "no_fold": {"PSIGNN_U2D_KMAX": "0"},
    "two_pass": {"PSIGNN_UVU": "0"},
    "lds_max": {"PSIGNN_U2D_FORM": "lds", "PSIGNN_U2D_KMAX": "31", "PSIGNN_U2D_KEEP": "31"},
}
W = 3 << 18          # the width switch: 16 floats per lane from here up
REG = 2047 * 1024    # cdiv(M, 1024) >= 2048, the register fold, above this length


def case(name, M, thr, env=None, hist=0, keep_trace=1, hex_n=0, shard=0):
    """hex_n > 0: a handle on the plan of make_hex_problem(hex_n) (M, n_tiles follow from it); shard: shard_elems = shard * M."""
    return dict(case=name, M=M, thr=thr, env=dict(env or {}), hist=hist, keep_trace=keep_trace, hex_n=hex_n, shard=shard)


def cases():
    cs = [
        case("m10", 10, 6),                                         # less than a quad of lanes
        case("m4090", 4090, 36),                                    # two-pass form, 4 floats per lane, partial last block; combine from k = 32
        case("m4090_jgroups2", 4090, 12, {"PSIGNN_JGROUPS": "2"}),  # split over 2 pair groups from k = 8
        case("m4090_vec16", 4090, 12, {"PSIGNN_VEC16_MIN": "1000"}),
        case("m4090_bf16", 4090, 12, hist=1),
        case("below_width_switch", W - 1, 12),
        case("width_switch", W, 28),                                # three-sweep form at width 4; the fold crosses k = 24 into the window
        case("width_switch_no_trace", W, 12, keep_trace=0),
        case("mid_vec16_min_above", 1000000, 12, {"PSIGNN_VEC16_MIN": "2000000"}),
        case("mid_ragged", 1000010, 28),
        case("mid_vec_ax4_0", 1000000, 28, {"PSIGNN_VEC_AX4": "0"}),   # 16 floats per lane, split axpy pass and its combine launch
        case("mid_bf16", 1000000, 28, hist=1),
        case("below_reg_fold", REG, 28),
        case("above_reg_fold", REG + 1, 28),                        # register fold: KB = 8 / 16 / 24
        case("long", 3200000, 28),                                  # jgroups = 1, 16 floats per lane
        case("long_vec_ax4_1", 3200000, 12, {"PSIGNN_VEC_AX4": "1"}),
        case("long_two_pass", 3200000, 12, {"PSIGNN_UVU": "0"}),
        case("long_bf16", 3200000, 12, hist=1),
        case("long_lds", 3200000, 28, {"PSIGNN_U2D_FORM": "lds"}),
        case("ask_38", 1000000, 48, {"PSIGNN_U2D_FORM": "lds", "PSIGNN_U2D_KMAX": "38", "PSIGNN_U2D_KEEP": "36"}),
        case("plan_hex13", 0, 12, hex_n=13),                        # plan-order inputs and the f workspace; no size hint
        case("plan_hex58", 0, 28, hex_n=58),
        case("short_shard", 0, 28, hex_n=58, shard=8),              # size_hint > M: 16 floats per lane, 4 pair groups, axpy at width 4
        case("short_shard_two_pass", 0, 28, {"PSIGNN_UVU": "0"}, hex_n=58, shard=8),
        case("short_shard_reg", 0, 28, hex_n=58, shard=24),         # a shard long enough for the register fold
        case("small_shard", 0, 12, hex_n=13, shard=3),              # size_hint > M below the width switch
    ]
    cs += [case(f"mid_{n}", 1000000, 48, e) for n, e in ENVS.items()]   # lds_max at 48: keep0 > 0 in the LDS form
    cs += [case(f"long_{n}", 3200000, 28, e) for n, e in ENVS.items() if n in ("keep8", "window_from_5", "no_fold")]
    return cs


def linear(M, dev, seq):
    gen = torch.Generator().manual_seed(0)
    c = 0.05 + 0.945 * torch.rand(M // seq, seq, generator=gen)
    b = torch.randn(M // seq, seq, generator=gen)
    x0 = torch.randn(M // seq, seq, generator=gen)
    return c.to(dev), b.to(dev), x0.to(dev)


def make_solver(cs, dev):
    """(solver, M, size_hint, plan nodes, n_tiles, seq_len) of a case; the caller has set the environment."""
    eng = pkg("engine")
    if cs["hex_n"]:
        mesh = pkg("data").make_hex_problem(cs["hex_n"], seed=0, compute_sol=False)
        plan = eng.MeshPlan(mesh.to(dev))
        M = int(plan.N) * 10
        sv = eng.DeviceBroyden(plan=plan, threshold=cs["thr"], keep_trace=bool(cs["keep_trace"]), shard_elems=cs["shard"] * M)
        tiles = int(plan.export("tile_ptr").shape[0] - 1) if plan.tiled else 0
        return sv, M, cs["shard"] * M, int(plan.N), tiles, 10
    M = cs["M"]
    seq = 10 if M % 10 == 0 else 1
    sv = eng.DeviceBroyden(threshold=cs["thr"], keep_trace=bool(cs["keep_trace"]), n_elems=M, seq_len=seq, device=dev,
                           history_dtype=torch.bfloat16 if cs["hist"] else torch.float32)
    return sv, M, 0, 0, 0, seq


def run_case(cs, dev):
    """The row of a case and the solve's output dict."""
    nat = pkg("_native")
    saved = {k: os.environ.pop(k, None) for k in KNOBS}
    os.environ.update(cs["env"])
    try:
        sv, M, hint, nodes, tiles, seq = make_solver(cs, dev)
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    c, b, x0 = linear(M, dev, seq)
    nat.prof_enable(True)
    nat.prof_collect()
    try:
        out = sv.solve_callable(lambda x: c * x + b, x0, 0.0)
        nat.prof_collect(with_bytes=True)
        log = nat.prof_launch_log()
    finally:
        nat.prof_enable(False)
    assert out["n_iter"] == cs["thr"], (cs["case"], out["n_iter"])
    iters = []
    for name, _, byts in log:
        if name == "k_resid":                     # launch_update: the head of every iteration of a host-driven solve
            iters.append([])
        elif name in CHAIN:
            assert byts % M == 0, (cs["case"], name, byts)
            iters[-1].append([name, byts // M])
    assert len(iters) == cs["thr"], (cs["case"], len(iters))
    row = {"case": cs["case"], "M": M, "size_hint": hint, "thr": cs["thr"], "hist": cs["hist"], "keep_trace": cs["keep_trace"],
           "plan_nodes": nodes, "n_tiles": tiles, "env": cs["env"], "nbytes": sv.nbytes, "iters": iters}
    sv.close()
    return row, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "record_broyden_schedule.py needs a GPU"
    dev = torch.device("cuda:0")
    rows = [json.dumps(run_case(cs, dev)[0], separators=(",", ":")) for cs in cases()]
    text = "[\n" + ",\n".join(rows) + "\n]\n"      # one row per line: the host check reads it line by line
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    print(f"{len(rows)} cases, {len(text)} bytes")


if __name__ == "__main__":
    main()
