"""CPU: the float64 derivative products (``psignn_f64_jvp``, ``psignn_f64_vjp``, ``psignn_f64_deriv_workspace_doubles``;
``engine.FixedPointMap64.jvp`` / ``.vjp``) -- the C ABI surface and every refusal that needs no device."""
import ctypes
import inspect
import os
import re
import types

import pytest
import torch

from conftest import ROOT, pkg

NEW = {"psignn_f64_jvp": 12, "psignn_f64_vjp": 13, "psignn_f64_deriv_workspace_doubles": 3}


def test_entries_in_header_table_and_default_library_only():
    nat = pkg("_native")
    hdr = open(os.path.join(ROOT, "include", "psignn_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    decl = dict(re.findall(r"\b(psignn_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", hdr))
    lib = ctypes.CDLL(nat.LIB_PATH)
    for name, arity in NEW.items():
        assert name in decl, name
        assert decl[name].count(",") + 1 == arity, (name, decl[name])
        assert len(nat.SIGNATURES[name][1]) == arity, name
        assert hasattr(lib, name), name
    for w in (8, 16):   # default-width library only
        raw = ctypes.CDLL(nat.lib_path(w))
        assert not any(hasattr(raw, n) for n in NEW), w


def test_every_entry_has_an_integration_row_citing_the_reference():
    rows = [l for l in open(os.path.join(ROOT, "INTEGRATION.md")).read().splitlines() if l.startswith("|")]
    for name in NEW:
        hits = [l for l in rows if name in l]
        assert hits and any("model.py:210-225" in l for l in hits), name


def test_python_signatures():
    eng = pkg("engine")
    sig = lambda f: inspect.signature(f).parameters
    assert list(sig(eng.FixedPointMap64.jvp)) == ["self", "H", "V"]
    p = sig(eng.FixedPointMap64.vjp)
    assert list(p) == ["self", "H", "Wv", "add"] and p["add"].default is None


def _hand_made(handle=1):
    """A map filled in by hand around a handle that is never used: the checks under test come before any native call."""
    eng = pkg("engine")
    fm = eng.FixedPointMap64.__new__(eng.FixedPointMap64)
    fm.plan = types.SimpleNamespace(mixed=False, N=7, E=20, device=torch.device("cpu"), handle=None)
    fm.handle, fm.device = handle, torch.device("cpu")
    return fm


def test_wrong_shapes_and_closed_handles():
    nat = pkg("_native")
    fm = _hand_made()
    ok = torch.zeros(7, 10)
    for shape in ((7, 8), (6, 10), (70,)):
        bad = torch.zeros(*shape)
        with pytest.raises(nat.NativeError, match="H has shape"):
            fm.jvp(bad, ok)
        with pytest.raises(nat.NativeError, match="H has shape"):
            fm.vjp(bad, ok)
        with pytest.raises(nat.NativeError, match="V has shape"):
            fm.jvp(ok, bad)
        with pytest.raises(nat.NativeError, match="Wv has shape"):
            fm.vjp(ok, bad)
        with pytest.raises(nat.NativeError, match="add has shape"):
            fm.vjp(ok, ok, bad)
    # shapes right, tensors on the host: there is no CPU route
    with pytest.raises(nat.NativeError, match="device tensors"):
        fm.jvp(ok, ok)
    with pytest.raises(nat.NativeError, match="device tensors"):
        fm.vjp(ok, ok)
    fm.handle = None
    with pytest.raises(nat.NativeError, match="closed"):
        fm.jvp(ok, ok)
    with pytest.raises(nat.NativeError, match="closed"):
        fm.vjp(ok, ok)


def test_null_arguments_are_error_codes():
    nat = pkg("_native")
    lib = nat.lib()
    assert lib.psignn_f64_jvp(None, None, 1, None, None, None, None, None, None, None, 0, None) < 0
    assert "NULL" in lib.psignn_last_error().decode()
    assert lib.psignn_f64_vjp(None, None, 1, None, None, None, None, None, None, None, None, 0, None) < 0
    assert "NULL" in lib.psignn_last_error().decode()
    assert lib.psignn_f64_deriv_workspace_doubles(None, 1, 0) == -1
    assert lib.psignn_f64_deriv_workspace_doubles(None, 1, 1) == -1
