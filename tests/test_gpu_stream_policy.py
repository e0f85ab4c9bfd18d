"""The memory policy of a load or a store must not change a bit.

The Broyden sweeps and the fused f tile kernel give data that is touched once per iteration (the stored pairs U_j, V_j, the new
pair, the slot records) a streaming policy, under conditions: the sweeps at 16 floats per lane only (the long form), the register
fold from 2M floats, the slot records in the fused dirichlet step.  Same operations in the same order on every element: each solve
below is compared with tests/golden/stream_policy_parent.npz, recorded by scripts/record_stream_policy_golden.py on the commit
before the policy change.  That script's docstring lists the cases and which helper each one runs: ``long_form`` is the one that
launches ``k_sweep_u1<16>`` / ``k_sweep_v<16>`` (``ldv_stream<16>``, ``stv_stream<16>`` with a ragged tail), ``reg_fold`` and
``long_form`` run the register fold's ``ld4_so_stream`` / ``st4_so_stream``, the two ``gnn_*`` cases the slot loads; the others run
the helpers' plain branches and the forms that were to stay as they were.  Every trace entry and every stored row must be EQUAL,
bit for bit: a helper that drops a ragged tail, mixes up a row offset or narrows a store shows up here in the first iteration."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, pkg

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("record_stream_policy_golden", os.path.join(ROOT, "scripts", "record_stream_policy_golden.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(GOLDEN, "stream_policy_parent.npz")))


@pytest.mark.parametrize("case", rec.CASES)
def test_solve_keeps_the_parent_bits(case, golden, dev, monkeypatch):
    for k in rec.KNOBS:
        monkeypatch.delenv(k, raising=False)
    pkg("_native").lib().psignn_reload_knobs()
    got = rec.run_case(case, dev)
    want = {k[len(case) + 1:]: v for k, v in golden.items() if k.startswith(case + ".")}
    assert sorted(got) == sorted(want) and len(want) == 10, (sorted(got), sorted(want))
    assert np.array_equal(got["rows"], want["rows"])
    for k in sorted(want):
        if k in ("rel_trace", "abs_trace"):     # float64 values: compared as bit patterns too (a NaN would equal itself)
            assert np.array_equal(got[k].view(np.uint64), want[k].view(np.uint64)), (case, k)
        elif k != "rows":
            assert got[k].dtype == np.uint32 and want[k].dtype == np.uint32
            assert np.array_equal(got[k], want[k]), (case, k, int((got[k] != want[k]).sum()))
