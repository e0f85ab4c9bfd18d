"""``broyden_stop_ref.replay`` against the CPU oracle's Broyden solver on every scripted case, before the GPU tests use it as a judge.

``oracle.broyden`` is the bit-for-bit restatement of the reference's solver (utilities/solver.py:116-207).  Every case of
``broyden_stop_ref.CASES`` runs through it in fp32 and with a float64 default dtype, in both stop modes: what ``replay`` says of
the returned traces -- the step at which the loop ends, the lowest value and its step, ``prot_break``, both padded traces -- must
equal what the oracle returned, the stop must be the one the case names (all four reasons and every boundary of the table), and
``result`` must be, bit for bit, the x handed to call ``nstep`` of the scripted map."""
import numpy as np
import pytest
import torch

import broyden_stop_ref as bsr
from oracle import psignn_oracle as orc


@pytest.fixture(params=["float32", "float64"])
def dtype(request):
    dt = getattr(torch, request.param)
    before = torch.get_default_dtype()
    torch.set_default_dtype(dt)      # (the oracle allocates its pairs in the default dtype, like the reference)
    yield dt
    torch.set_default_dtype(before)


def _oracle(stop_mode):
    def solve(f, x0, threshold, eps):
        with torch.no_grad():
            return orc.broyden(f, x0, threshold=threshold, eps=eps, stop_mode=stop_mode)
    return solve


@pytest.mark.parametrize("stop_mode", ["rel", "abs"])
@pytest.mark.parametrize("shape", [(16, 10), (409, 10), (16, 7), (409, 7)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_replay_is_the_oracles_stop_decision(shape, stop_mode, dtype):
    x0 = bsr.start_vector(shape, dtype=dtype)
    seen = set()
    for case in bsr.cases_for(shape[1], stop_mode):
        out, sc, rp = bsr.run_case(case, _oracle(stop_mode), x0, stop_mode)
        # the script is what the solver saw: each entry within half of the smallest margin of the table (0.8 %, a ratio of two entries)
        tr = np.array(out[stop_mode + "_trace"][:rp["n_iter"]])
        want = np.array(sc.values[1:rp["n_iter"] + 1] + sc.values[-1:] * max(0, rp["n_iter"] + 1 - len(sc.values)))
        want = want * (sc.x0_norm if stop_mode == "abs" else 1.0)
        assert np.max(np.abs(tr / want - 1)) < (4e-3 if dtype == torch.float32 else 1e-9), (case.name, np.max(np.abs(tr / want - 1)))
        assert len(out["xest_trace"]) == rp["n_iter"] + 1 and torch.equal(out["xest_trace"][out["nstep"]], out["result"])
        seen.add(rp["stop_reason"])
    assert seen == {0, 1, 2, 3}


def test_replay_reports_a_stop_no_rule_explains():
    """A solve that ends one step early or runs one step late does not pass ``assert_replay``."""
    x0 = bsr.start_vector((16, 10))
    case = bsr.CASE["stagnation_at_31"]
    sc = bsr.Script(case.values(10, "rel"), "rel", x0)
    with torch.no_grad():
        out = orc.broyden(sc, x0, threshold=45, eps=case.eps)
    assert sc.calls - 1 == 31
    bsr.assert_replay(out, case.eps, 45, 10, "rel", n_iter=31)
    with pytest.raises(AssertionError, match="no rule fires"):
        bsr.assert_replay(out, case.eps, 45, 10, "rel", n_iter=30)
    late = dict(out, rel_trace=out["rel_trace"][:31] + [out["rel_trace"][30]] * 15, abs_trace=out["abs_trace"][:31] + [out["abs_trace"][30]] * 15)
    with pytest.raises(AssertionError, match="another step"):
        bsr.assert_replay(late, case.eps, 45, 10, "rel", n_iter=32)
    # the width reaches the break's limit: the same traces replayed at d = 10 and d = 7
    case = bsr.CASE["seq_len_7_breaks"]
    x7 = bsr.start_vector((16, 7))
    sc = bsr.Script(case.values(7, "rel"), "rel", x7)
    with torch.no_grad():
        out = orc.broyden(sc, x7, threshold=45, eps=case.eps)
    assert bsr.replay(out["rel_trace"], out["abs_trace"], 5, case.eps, 45, 7)["stop_reason"] == 3
    assert bsr.replay(out["rel_trace"], out["abs_trace"], 5, case.eps, 45, 10)["stop_reason"] is None
