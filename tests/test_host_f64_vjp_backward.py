"""CPU: the float64 backward of the VJP (``psignn_f64_vjp_backward`` and its workspace query; ``engine.FixedPointMap64.vjp_backward``,
``engine.jac_loss_grad64``) -- the C ABI surface, the documented workspace size and every refusal that needs no device."""
import ctypes
import inspect
import os
import re
import types

import pytest
import torch

from conftest import ROOT, load_weights, pkg

NEW = {"psignn_f64_vjp_backward": 15, "psignn_f64_vjp_backward_workspace_doubles": 2}
CITE = "model.py:416-435"


def test_entries_in_header_table_and_default_library_only():
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
        # the comment in front of the declaration carries a replaces: line citing the reference
        head = raw_hdr[:re.search(r"^(int|int64_t) " + name + r"\(", raw_hdr, re.M).start()]
        comment = head[head.rindex("/*"):]
        assert "replaces:" in comment and CITE in comment, name
    for w in (8, 16):   # default-width library only
        raw = ctypes.CDLL(nat.lib_path(w))
        assert not any(hasattr(raw, n) for n in NEW), w


def test_every_entry_has_an_integration_row_citing_the_reference():
    rows = [l for l in open(os.path.join(ROOT, "INTEGRATION.md")).read().splitlines() if l.startswith("|")]
    for name in NEW:
        hits = [l for l in rows if name in l]
        assert hits and any(CITE in l for l in hits), name


def test_python_signatures():
    eng = pkg("engine")
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(eng.FixedPointMap64.vjp_backward) == ["self", "H", "V", "Gbar"]
    assert sig(eng.FixedPointMap64.vjp_backward) == sig(eng.FixedPointMap.vjp_backward)[:4]
    assert sig(eng.jac_loss_grad64) == ["batch", "state_dict", "h_star", "probes"]


def test_workspace_query_without_a_handle():
    lib = pkg("_native").lib()
    q = lib.psignn_f64_vjp_backward_workspace_doubles
    assert q(None, 1) == -1 and q(None, 0) == -1
    assert q(1, 0) == -1 and q(1, -3) == -1   # n_layers < 1: refused before the handle is looked at
    assert lib.psignn_f64_vjp_backward(None, None, 1, None, None, None, None, None, None, None, None, None, None, 0, None) < 0
    assert "NULL" in lib.psignn_last_error().decode()


def _documented_size(N, nl, mixed, chunk, wsize1):
    """The header's formula: (loc, C) and their tangents, for a dirichlet chain the states, their tangents and two ping-pongs, then one
    partial row per chunk."""
    cw = 3 if mixed else 2
    chain = (not mixed) and nl > 1
    return N * 10 * (2 + 2 * cw) + (N * 10 * (2 * (nl - 1) + 4) if chain else 0) + -(-N // chunk) * wsize1


def test_workspace_size_is_positive_and_grows_with_depth_as_documented():
    """The documented formula, evaluated on the host: positive for every N >= 1, strictly growing with n_layers on a dirichlet block
    (two more (N, 10) arrays per layer) and independent of it on a mixed block, which differentiates its last layer alone.  The GPU
    test compares the native query with this function on open handles."""
    lib = pkg("_native").lib()
    chunk = int(lib.psignn_f64_param_vjp_chunk_rows())
    for mixed in (False, True):
        w1 = int(lib.psignn_f64_weights_size(int(mixed), 1))
        for N in (1, 127, 128, 129, 10981):
            sizes = [_documented_size(N, nl, mixed, chunk, w1) for nl in (1, 2, 3, 4)]
            assert all(s > 0 for s in sizes)
            if mixed:
                assert len(set(sizes)) == 1
            else:
                assert sizes[1] - sizes[0] == 6 * N * 10 and sizes[2] - sizes[1] == sizes[3] - sizes[2] == 2 * N * 10


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
    for shape in ((7, 8), (7, 16), (6, 10), (70,)):
        bad = torch.zeros(*shape)
        with pytest.raises(nat.NativeError, match="H has shape"):
            fm.vjp_backward(bad, ok, ok)
        with pytest.raises(nat.NativeError, match="V has shape"):
            fm.vjp_backward(ok, bad, ok)
        with pytest.raises(nat.NativeError, match="Gbar has shape"):
            fm.vjp_backward(ok, ok, bad)
    with pytest.raises(nat.NativeError, match="device tensors"):   # shapes right, tensors on the host: there is no CPU route
        fm.vjp_backward(ok, ok, ok)
    fm.handle = None
    with pytest.raises(nat.NativeError, match="closed"):
        fm.vjp_backward(ok, ok, ok)


def test_jac_loss_grad64_refusals_without_a_device():
    nat, eng = pkg("_native"), pkg("engine")
    sd = load_weights("dirichlet")
    batch = types.SimpleNamespace(x=torch.zeros(7, 4))
    ok = torch.zeros(7, 10)
    for bad in (torch.zeros(7, 8), torch.zeros(6, 10)):
        with pytest.raises(nat.NativeError, match="h_star has shape"):
            eng.jac_loss_grad64(batch, sd, bad, [ok])
        with pytest.raises(nat.NativeError, match="probe 1 has shape"):
            eng.jac_loss_grad64(batch, sd, ok, [ok, bad])
    with pytest.raises(nat.NativeError, match="probe 0 has shape"):
        eng.jac_loss_grad64(batch, sd, ok, torch.zeros(2, 7, 8))
    with pytest.raises(nat.NativeError, match="at least one probe"):
        eng.jac_loss_grad64(batch, sd, ok, [])
    for w in (8, 16):   # a state dict of another latent width: forward inference only
        wide = {"deqdss.f.laynorm.weight": torch.zeros(w)}
        with pytest.raises(nat.NativeError, match="forward inference only"):
            eng.jac_loss_grad64(batch, wide, ok, [ok])
