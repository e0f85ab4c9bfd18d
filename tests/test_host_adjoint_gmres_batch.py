"""CPU: the surface of the lockstep GMRES adjoint solve (C ABI, ctypes table, config keys, the host-side route decision); no
compute calls -- there is no GPU here."""
import ctypes
import inspect
import os
import re
import types

import pytest
import torch

from conftest import ROOT, pkg

NEW = {"psignn_gmres_create_for_batch": 6, "psignn_gmres_adjoint_batchable": 3, "psignn_gmres_solve_adjoint_lin_batch": 15}


def test_new_entries_in_header_table_and_library():
    nat = pkg("_native")
    raw_hdr = open(os.path.join(ROOT, "include", "psignn_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw_hdr, flags=re.S)
    decl = dict(re.findall(r"\b(psignn_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", hdr))
    lib = ctypes.CDLL(nat.LIB_PATH)
    for name, arity in NEW.items():
        assert name in decl, name
        assert decl[name].count(",") + 1 == arity, (name, decl[name])
        assert len(nat.SIGNATURES[name][1]) == arity, name
        assert hasattr(lib, name), name
        # documented like its neighbours: the comment in front of the declaration cites what it replaces in the reference
        doc = raw_hdr[:raw_hdr.index("int " + name + "(")].rsplit("/*", 1)[1]
        assert "replaces:" in doc and "main.py:106" in doc and "model.py:210-223" in doc, name
    # the width libraries do not build the Krylov file: none of the entries is in them
    for w in (8, 16):
        raw = ctypes.CDLL(nat.lib_path(w))
        assert not any(hasattr(raw, n) for n in NEW)
    # a host-side question: 0 for an empty shard and for NULL arguments, nothing touched
    L = nat.lib()
    one = (ctypes.c_void_p * 1)(None)
    assert L.psignn_gmres_adjoint_batchable(0, None, None) == 0
    assert L.psignn_gmres_adjoint_batchable(2, None, None) == 0
    assert L.psignn_gmres_adjoint_batchable(1, one, None) == 0
    assert L.psignn_gmres_adjoint_batchable(1, one, one) == 0


def test_integration_table_names_the_entries():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW:
        row = [ln for ln in doc.splitlines() if ln.startswith("|") and name in ln]
        assert row, name
        assert "main.py:106" in row[0] and "model.py:210-223" in row[0]


def test_python_surface():
    eng = pkg("engine")
    sig = inspect.signature(eng.DeviceGmres.__init__)
    assert list(sig.parameters) == ["self", "n_elems", "device", "m_max", "shard_elems"]
    assert sig.parameters["shard_elems"].default is None
    assert list(inspect.signature(eng.gmres_adjoint_batchable).parameters) == ["solvers", "lins"]
    sig = inspect.signature(eng.gmres_solve_adjoint_batch)
    assert list(sig.parameters) == ["solvers", "lins", "grads", "eps", "max_products", "poll_every"]
    assert sig.parameters["poll_every"].default == 8
    assert eng.gmres_adjoint_batchable([], []) is False
    assert eng.gmres_solve_adjoint_batch([], [], [], 1e-6, 10) == []
    assert list(inspect.signature(pkg("model_psignn")._ReplicaSlot.gmres).parameters) == ["self", "plan", "m", "shard_elems"]


@pytest.mark.parametrize("mod", ["model_psignn", "mixed"])
def test_lockstep_key(mod):
    nat = pkg("_native")
    mk = lambda **kw: pkg(mod).ModelDEQDSS(dict(latent_dim=10, n_layers=1, bw_thres=40, **kw))
    # off by default
    assert not mk().config_deq.get("bw_gmres_lockstep", False)
    assert not mk(bw_solver="gmres").config_deq.get("bw_gmres_lockstep", False)
    assert mk(bw_solver="gmres", bw_gmres_lockstep=False).config_deq["bw_gmres_lockstep"] is False
    net = mk(bw_solver="gmres", bw_gmres_lockstep=True)
    assert net.config_deq["bw_gmres_lockstep"] is True and net.config_deq["bw_gmres_m"] == 40
    # True needs bw_solver = "gmres": the error names both keys
    for kw in (dict(), dict(bw_solver=None)):
        with pytest.raises(nat.NativeError, match="bw_gmres_lockstep.*bw_solver"):
            mk(bw_gmres_lockstep=True, **kw)
    assert mk(bw_gmres_lockstep=False).config_deq["bw_gmres_lockstep"] is False   # False asks for nothing
    with pytest.raises(nat.NativeError, match="bw_gmres_lockstep must be a bool"):
        mk(bw_solver="gmres", bw_gmres_lockstep=1)


def _stub(tiled=True, n_layers=1, mixed=False, lin_neumann="direct", linearizable=True):
    return types.SimpleNamespace(plan=types.SimpleNamespace(tiled=tiled, mixed=mixed), weights=types.SimpleNamespace(n_layers=n_layers),
                                 can_linearize=lambda: linearizable, lin_neumann=lin_neumann)


def test_lockstep_applies_with_the_key():
    mk = lambda **kw: pkg("model_psignn").ModelDEQDSS(dict(latent_dim=10, n_layers=1, **kw)).deqdss
    on = mk(bw_solver="gmres", bw_gmres_lockstep=True)
    # the early return is gone: the maps decide
    assert on.lockstep_applies([_stub(), _stub()]) is True
    assert on.lockstep_applies([_stub(mixed=True, lin_neumann="stored")] * 2) is True
    assert on.lockstep_applies([_stub(), _stub(tiled=False)]) is False
    assert on.lockstep_applies([_stub(n_layers=2)]) is False
    assert on.lockstep_applies([_stub(linearizable=False)]) is False
    assert on.lockstep_applies([_stub(mixed=True)]) is False                       # mixed without lin_neumann = "stored"
    assert on.lockstep_applies([_stub(), _stub(mixed=True, lin_neumann="stored")]) is False   # both families
    # key false or absent: still decided before the maps are looked at
    for off in (mk(bw_solver="gmres"), mk(bw_solver="gmres", bw_gmres_lockstep=False)):
        assert off.lockstep_applies([object()]) is False
        assert off.lockstep_applies([_stub()]) is False
    # without bw_solver the Broyden lockstep is what it was
    assert mk().lockstep_applies([_stub()]) is True


@pytest.mark.parametrize("d", [8, 16])
def test_other_widths_stay_forward_only_with_both_keys(d, monkeypatch):
    nat = pkg("_native")
    net = pkg("model_psignn").ModelDEQDSS(dict(latent_dim=d, n_layers=1, bw_solver="gmres", bw_gmres_lockstep=True))
    monkeypatch.setattr(nat, "lib", lambda *a: (_ for _ in ()).throw(AssertionError("the library was touched")))
    deq = net.deqdss
    for call in (lambda: net.train()([object(), object()]), lambda: deq.train_forward(torch.zeros(3, d), object()),
                 lambda: deq.implicit_backward(None, None, object(), torch.zeros(3, d)),
                 lambda: deq.train_forward_replicas([torch.zeros(3, d)] * 2, [object()] * 2)):
        with pytest.raises(nat.NativeError, match=f"latent_dim {d} has forward inference only"):
            call()
