"""csrc/solver_shapes.h against the recorded Broyden schedule (tests/golden/broyden_schedule.json, scripts/record_broyden_schedule.py).

tests/host/solver_shapes_check.cpp includes only solver_shapes.h; it is compiled with the host compiler under AddressSanitizer
and UBSan and run on its own: for every row of the table it derives the handle's shape from the row's sizes and knobs, runs the
update chain on a recording target for ``thr`` iterations and prints the bytes the shape allocates and the passes with their
stated bytes; it also asserts the fold's limits (kept pairs within a row of partials, the LDS form's 38 / 36 = 31 / 31).  What
it prints is compared with the table here, in both directions."""
import json
import os
import shutil
import subprocess

import pytest

from conftest import GOLDEN, ROOT

TABLE = os.path.join(GOLDEN, "broyden_schedule.json")
SRC = os.path.join(ROOT, "tests", "host", "solver_shapes_check.cpp")
CSRC = os.path.join(ROOT, "psi-gnn_amd", "csrc")


@pytest.fixture(scope="module")
def table():
    with open(TABLE) as f:
        return {r["case"]: r for r in json.load(f)}


def test_table_takes_every_branch(table):
    """The forms the schedule can take all occur in some row: both widths, the two-pass form with and without the split and
    its combine launch, the three-sweep form plain, folded and in the window regime (a sweep 1 after a fold), bf16 pairs,
    plan handles, shard-sized handles."""
    names = {c: {n for it in r["iters"] for n, _ in it} for c, r in table.items()}
    assert 30 <= len(table) <= 40
    assert any("k_axpy_combine" in n for n in names.values()) and any("k_dots" in n and "k_axpy_combine" not in n for n in names.values())
    assert any("k_sweep_u2d" in n and "k_sweep_u1" in n for n in names.values())
    assert any("k_sweep_u2" in n and "k_sweep_u2d" not in n and "k_sweep_v" in n for n in names.values())
    assert any("k_sweep_v_bf16" in n for n in names.values())
    assert any(r["size_hint"] > r["M"] for r in table.values()) and any(r["n_tiles"] > 0 and r["size_hint"] == 0 for r in table.values())
    assert {3 << 18, (3 << 18) - 1, 10, 4090, 2047 * 1024, 2047 * 1024 + 1} <= {r["M"] for r in table.values()}
    for r in table.values():
        assert len(r["iters"]) == r["thr"]


def test_shapes_and_schedule_match_the_table(table, tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "solver_shapes_check")
    # the sanitizer runtimes are linked into the program (clang's default): it runs on its own, whatever else the process loads
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *static,
                    "-I", CSRC, SRC, "-o", exe], check=True)
    r = subprocess.run([exe, TABLE], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    got = {x["case"]: x for x in map(json.loads, (ln for ln in r.stdout.splitlines() if ln.startswith("{")))}
    assert sorted(got) == sorted(table)
    for c, row in table.items():
        assert got[c]["nbytes"] == row["nbytes"], c
        assert got[c]["iters"] == row["iters"], c
