"""csrc/workspace.h against the recorded workspace sizes (tests/golden/workspace_sizes.json, oracle/make_golden_workspace_sizes.py).

tests/host/workspace_check.cpp includes only workspace.h; it is compiled with the host compiler under AddressSanitizer and
UBSan, once per latent width, and run on its own: every segment of every layout inside its total, no overlap outside the declared
aliases, even offsets, and every total equal to the recorded value of its query.  The totals it prints are compared with the table
here, in both directions."""
import json
import os
import shutil
import subprocess

import pytest

from conftest import GOLDEN, ROOT, pkg

TABLE = os.path.join(GOLDEN, "workspace_sizes.json")
SRC = os.path.join(ROOT, "tests", "host", "workspace_check.cpp")
CSRC = os.path.join(ROOT, "psi-gnn_amd", "csrc")
NS = [1, 63, 64, 65, 257, 5329, 99919, 1000519]
NLS = [1, 2, 3, 64]


def _key(r):
    return (r["D"], r["query"], r["mixed"], r["nl"], r["N"])


@pytest.fixture(scope="module")
def table():
    with open(TABLE) as f:
        return {_key(r): r["floats"] for r in json.load(f)}


def test_table_covers_the_stated_cases(table):
    per_plan = ["f", "f_param_vjp", "f_vjp_backward", "f_vjp_backward_p", "dsgps_step_backward", "dss_step_backward", "mlp2_backward"]
    for n in NS:
        for mixed in (0, 1):
            assert all((d, "f", mixed, 1, n) in table for d in (8, 10, 16))
            assert all((10, q, mixed, 1, n) in table for q in per_plan)
            assert all((10, q, mixed, nl, n) in table for q in ("f_layers", "gmres_adjoint") for nl in NLS)


@pytest.mark.parametrize("width", [8, 10, 16])
def test_layouts_hold_and_totals_match_the_table(width, table, tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / f"workspace_check_d{width}")
    # the sanitizer runtimes are linked into the program (clang's default): it runs on its own, whatever else the process loads
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *static,
                    f"-DPSIGNN_D={width}", "-I", CSRC, SRC, "-o", exe], check=True)
    r = subprocess.run([exe, TABLE], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    got = {_key(x): x["floats"] for x in map(json.loads, (ln for ln in r.stdout.splitlines() if ln.startswith("{")))}
    want = {k: v for k, v in table.items() if k[0] == width}
    assert got == want


def test_library_queries_return_the_table(table):
    """The built library's plan-free query, and the arithmetic the table implies for it."""
    lib = pkg("_native").lib()
    for n in NS:
        assert int(lib.psignn_mlp2_backward_workspace_floats(n)) == table[(10, "mlp2_backward", 0, 1, n)]
