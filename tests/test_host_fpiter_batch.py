"""CPU: the surface of the lockstep Anderson / Picard solves (C ABI, ctypes table, INTEGRATION.md, the ``fp_lockstep`` config key and
the host-side route decision); no compute calls -- there is no GPU here."""
import ctypes
import inspect
import os
import re
import types

import pytest

from conftest import ROOT, pkg

NEW = {"psignn_fpiter_create_for_batch": 6, "psignn_fpiter_batchable": 3, "psignn_anderson_solve_batch": 19,
       "psignn_picard_solve_batch": 15}


def test_new_entries_in_header_table_and_libraries():
    nat = pkg("_native")
    raw_hdr = open(os.path.join(ROOT, "include", "psignn_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw_hdr, flags=re.S)
    decl = dict(re.findall(r"\b(psignn_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", hdr))
    for name, arity in NEW.items():
        assert name in decl, name
        assert decl[name].count(",") + 1 == arity, (name, decl[name])
        assert len(nat.SIGNATURES[name][1]) == arity, name
        # documented like its neighbours: the comment in front of the declaration cites what it replaces in the reference
        doc = raw_hdr[:raw_hdr.index("int " + name + "(")].rsplit("/*", 1)[1]
        assert "replaces:" in doc and "main.py:106" in doc, name
        # fpiter.hip is one of the forward translation units: all three libraries export the entries
        for w in (10, 8, 16):
            assert hasattr(ctypes.CDLL(nat.lib_path(w)), name), (name, w)


def test_integration_table_names_the_entries():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW:
        row = [ln for ln in doc.splitlines() if ln.startswith("|") and name in ln]
        assert row, name
        assert "main.py:106" in row[0] and "solver.py:215-293" in row[0] and ":301-341" in row[0]


@pytest.mark.parametrize("w", [10, 8, 16])
def test_host_side_answers_without_a_device(w):
    """``psignn_fpiter_batchable`` is a question: 0 for an empty shard and for NULL arrays.  The solves refuse the same arguments
    with an error code before anything is allocated or launched."""
    L = pkg("_native").lib(w)
    one = (ctypes.c_void_p * 1)(None)
    assert L.psignn_fpiter_batchable(0, None, None) == 0
    assert L.psignn_fpiter_batchable(0, one, one) == 0
    assert L.psignn_fpiter_batchable(2, None, None) == 0
    assert L.psignn_fpiter_batchable(1, one, None) == 0
    assert L.psignn_fpiter_batchable(1, one, one) == 0
    tail_a = (1e-4, 1.0, 0, 0.0, 8, None, None, None, None, None, None)
    tail_p = (1e-5, 8, None, None, None, None, None)
    assert L.psignn_anderson_solve_batch(0, None, None, None, 1, None, None, None, *tail_a) != 0
    assert L.psignn_anderson_solve_batch(2, None, None, None, 1, None, None, None, *tail_a) != 0
    assert L.psignn_anderson_solve_batch(1, one, one, None, 1, one, one, None, *tail_a) != 0
    assert L.psignn_picard_solve_batch(0, None, None, None, 1, None, None, None, *tail_p) != 0
    assert L.psignn_picard_solve_batch(1, one, one, None, 1, one, one, None, *tail_p) != 0


def test_python_surface():
    eng, slv = pkg("engine"), pkg("utilities.solver")
    sig = inspect.signature(eng.DeviceFixedPointIter.__init__)
    assert list(sig.parameters) == ["self", "n_elems", "device", "m", "threshold", "keep_trace", "width", "shard_elems"]
    assert sig.parameters["shard_elems"].default is None
    assert list(inspect.signature(eng.fpiter_batchable).parameters) == ["iters", "fmaps"]
    sig = inspect.signature(eng.anderson_solve_batch)
    assert list(sig.parameters) == ["iters", "fmaps", "eps", "lam", "beta", "stop_mode", "poll_every"]
    assert [sig.parameters[k].default for k in ("lam", "beta", "stop_mode", "poll_every")] == [1e-4, 1.0, "rel", 8]
    sig = inspect.signature(eng.picard_solve_batch)
    assert list(sig.parameters) == ["iters", "fmaps", "eps", "poll_every"] and sig.parameters["poll_every"].default == 8
    sig = inspect.signature(slv.anderson_batch)
    assert list(sig.parameters) == ["fmaps", "m", "lam", "threshold", "eps", "stop_mode", "beta", "poll_every"]
    assert [p.default for p in list(sig.parameters.values())[1:]] == [2, 1e-4, 50, 1e-3, "rel", 1.0, 8]
    sig = inspect.signature(slv.forward_iteration_batch)
    assert list(sig.parameters) == ["fmaps", "eps", "threshold", "poll_every"]
    assert [p.default for p in list(sig.parameters.values())[1:]] == [1e-5, 50, 8]
    # empty shards: a decision / an empty list, nothing touched
    assert eng.fpiter_batchable([], []) is False
    assert eng.anderson_solve_batch([], [], 1e-3) == [] and eng.picard_solve_batch([], [], 1e-5) == []
    assert slv.anderson_batch([]) == [] and slv.forward_iteration_batch([]) == []
    with pytest.raises(ValueError, match="stop_mode"):
        slv.anderson_batch([], stop_mode="both")


@pytest.mark.parametrize("mod", ["model_psignn", "mixed"])
def test_fp_lockstep_key(mod):
    nat, slv = pkg("_native"), pkg("utilities.solver")
    mk = lambda **kw: pkg(mod).ModelPSIGNN(dict(latent_dim=10, n_layers=1, **kw))
    # off by default, with every solver
    assert not mk().config_deq.get("fp_lockstep", False)
    assert not mk(solver=slv.anderson).config_deq.get("fp_lockstep", False)
    assert mk(solver=slv.anderson, fp_lockstep=False).config_deq["fp_lockstep"] is False
    for s in (slv.anderson, slv.forward_iteration):
        assert mk(solver=s, fp_lockstep=True).config_deq["fp_lockstep"] is True
    # True needs one of the two solvers: the error names both keys
    for kw in (dict(), dict(solver=slv.broyden), dict(solver=slv.newton)):
        with pytest.raises(nat.NativeError, match="fp_lockstep.*solver"):
            mk(fp_lockstep=True, **kw)
    assert mk(solver=slv.broyden, fp_lockstep=False).config_deq["fp_lockstep"] is False   # False asks for nothing
    with pytest.raises(nat.NativeError, match="fp_lockstep must be a bool"):
        mk(solver=slv.anderson, fp_lockstep=1)


def _stub(tiled=True, n_layers=1, mixed=False):
    return types.SimpleNamespace(plan=types.SimpleNamespace(tiled=tiled, mixed=mixed), weights=types.SimpleNamespace(n_layers=n_layers))


def test_fp_lockstep_applies_is_a_host_decision():
    slv = pkg("utilities.solver")
    mk = lambda **kw: pkg("model_psignn").ModelDEQDSS(dict(latent_dim=10, n_layers=1, **kw)).deqdss
    on = mk(solver=slv.anderson, fp_lockstep=True)
    assert on.fp_lockstep_applies([_stub(), _stub()]) is True
    assert on.fp_lockstep_applies([_stub(mixed=True)] * 3) is True
    assert on.fp_lockstep_applies([_stub()]) is False                              # one mesh: nothing to batch
    assert on.fp_lockstep_applies([_stub(), _stub(tiled=False)]) is False
    assert on.fp_lockstep_applies([_stub(), _stub(n_layers=2)]) is False
    assert on.fp_lockstep_applies([_stub(), _stub(mixed=True)]) is False           # both families
    # key false or absent: decided before the maps are looked at
    for off in (mk(solver=slv.anderson), mk(solver=slv.anderson, fp_lockstep=False), mk()):
        assert off.fp_lockstep_applies([object(), object()]) is False
    # the Broyden lockstep route does not look at the key
    assert mk(solver=slv.anderson, fp_lockstep=True).lockstep_applies([_stub(), _stub()]) is False
