"""CPU: the float64 parameter gradients (``psignn_f64_param_vjp``, ``psignn_mlp2_f64_backward`` and their queries;
``engine.FixedPointMap64.param_vjp``, ``mlp2_64_backward``, ``unpack_param_grads64``, ``implicit_grad64``) -- the C ABI surface and
every refusal that needs no device."""
import ctypes
import inspect
import os
import re
import types

import pytest
import torch

from conftest import ROOT, load_weights, pkg

NEW = {"psignn_f64_param_vjp": 14, "psignn_f64_param_vjp_workspace_doubles": 2, "psignn_f64_param_vjp_chunk_rows": 0,
       "psignn_mlp2_f64_backward": 14, "psignn_mlp2_f64_backward_workspace_doubles": 4}
CITES = {"psignn_f64_param_vjp": "model.py:203-225", "psignn_f64_param_vjp_workspace_doubles": "model.py:203-225",
         "psignn_f64_param_vjp_chunk_rows": "model.py:203-225", "psignn_mlp2_f64_backward": "model.py:370-392",
         "psignn_mlp2_f64_backward_workspace_doubles": "model.py:370-392"}


def test_entries_in_header_table_and_default_library_only():
    nat = pkg("_native")
    raw_hdr = open(os.path.join(ROOT, "include", "psignn_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw_hdr, flags=re.S)
    decl = dict(re.findall(r"\b(psignn_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", hdr))
    lib = ctypes.CDLL(nat.LIB_PATH)
    for name, arity in NEW.items():
        assert name in decl, name
        args = decl[name].strip()
        assert (0 if args == "void" else args.count(",") + 1) == arity, (name, decl[name])
        assert len(nat.SIGNATURES[name][1]) == arity, name
        assert hasattr(lib, name), name
        # the comment in front of the declaration carries a replaces: line citing the reference
        head = raw_hdr[:re.search(r"^(int|int64_t) " + name + r"\(", raw_hdr, re.M).start()]
        comment = head[head.rindex("/*"):]
        assert "replaces:" in comment and CITES[name] in comment, name
    for w in (8, 16):   # default-width library only
        raw = ctypes.CDLL(nat.lib_path(w))
        assert not any(hasattr(raw, n) for n in NEW), w


def test_every_entry_has_an_integration_row_citing_the_reference():
    rows = [l for l in open(os.path.join(ROOT, "INTEGRATION.md")).read().splitlines() if l.startswith("|")]
    for name in NEW:
        hits = [l for l in rows if name in l]
        assert hits and any(CITES[name] in l for l in hits), name


def test_python_signatures():
    eng = pkg("engine")
    sig = lambda f: inspect.signature(f).parameters
    p = sig(eng.FixedPointMap64.param_vjp)
    assert list(p) == ["self", "H", "Wv", "with_init"] and p["with_init"].default is True
    p = sig(eng.mlp2_64_backward)
    assert list(p) == ["x", "gy", "w1", "b1", "w2", "need_gx"] and p["need_gx"].default is True
    assert list(p) == list(sig(eng.mlp2_backward))
    p = sig(eng.unpack_param_grads64)
    assert list(p) == ["flat", "n_layers", "mixed"] == list(sig(eng.unpack_param_grads))
    p = sig(eng.implicit_grad64)
    assert list(p) == ["batch", "state_dict", "h_star", "grad", "solver", "eps", "m", "max_products", "threshold", "y"]
    want = {"solver": "gmres", "eps": 1e-11, "m": 50, "max_products": 2000, "threshold": 800, "y": None}
    assert {k: p[k].default for k in want} == want
    a = sig(eng.adjoint64)
    assert all(p[k].default == a[k].default for k in ("solver", "eps", "m", "max_products", "threshold"))


def _two_layer(mixed):
    torch.manual_seed(5)
    net = pkg("mixed" if mixed else "model_psignn").ModelPSIGNN(dict(latent_dim=10, n_layers=2))
    return {k: v.detach().clone() for k, v in net.state_dict().items()}


@pytest.mark.parametrize("mixed", [False, True])
def test_layout_length_and_round_trip(mixed):
    """``psignn_f64_weights_size`` is the length ``unpack_param_grads64`` expects, and unpacking the packed weights gives every
    ``deqdss.f.*`` tensor back, name for name and value for value."""
    nat, eng = pkg("_native"), pkg("engine")
    for nl in (1, 2, 3):
        size = int(nat.lib().psignn_f64_weights_size(int(mixed), nl))
        named = eng.unpack_param_grads64(torch.zeros(size, dtype=torch.float64), nl, mixed)
        assert sum(t.numel() for t in named.values()) == size
        for bad in (size - 1, size + 1):
            with pytest.raises(nat.NativeError, match="entries"):
                eng.unpack_param_grads64(torch.zeros(bad, dtype=torch.float64), nl, mixed)
    assert int(nat.lib().psignn_f64_weights_size(int(mixed), 1)) == (1924 if mixed else 1193)
    with pytest.raises(nat.NativeError, match="out of range"):
        eng.unpack_param_grads64(torch.zeros(4, dtype=torch.float64), 0, mixed)
    for sd in (load_weights("mixed" if mixed else "dirichlet"), _two_layer(mixed)):
        nl = eng.n_layers_of(sd)
        named = eng.unpack_param_grads64(eng.pack_weights64(sd), nl, mixed)
        want = {k[len("deqdss.f."):]: v for k, v in sd.items() if k.startswith("deqdss.f.")}
        assert set(named) == set(want) and len(named) == len(want)
        for k, v in want.items():
            assert named[k].shape == v.shape and torch.equal(named[k], v.double()), k
    names32 = list(eng.unpack_param_grads(torch.zeros(int(nat.lib().psignn_param_grad_size(int(mixed), 2))), 2, mixed))
    assert names32 == list(eng.unpack_param_grads64(torch.zeros(int(nat.lib().psignn_f64_weights_size(int(mixed), 2))), 2, mixed))


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
            fm.param_vjp(bad, ok)
        with pytest.raises(nat.NativeError, match="Wv has shape"):
            fm.param_vjp(ok, bad)
    with pytest.raises(nat.NativeError, match="device tensors"):   # shapes right, tensors on the host: there is no CPU route
        fm.param_vjp(ok, ok)
    fm.handle = None
    with pytest.raises(nat.NativeError, match="closed"):
        fm.param_vjp(ok, ok)


def test_engine_refusals_without_a_device():
    nat, eng = pkg("_native"), pkg("engine")
    with pytest.raises(nat.NativeError, match="device tensors"):
        eng.mlp2_64_backward(torch.zeros(3, 4), torch.zeros(3, 10), torch.zeros(10, 4), torch.zeros(10), torch.zeros(10, 10))
    sd = load_weights("dirichlet")
    batch = types.SimpleNamespace(x=torch.zeros(7, 4))
    ok = torch.zeros(7, 10)
    with pytest.raises(nat.NativeError, match="solver must be 'gmres' or 'broyden'"):
        eng.implicit_grad64(batch, sd, ok, ok, solver="anderson")
    with pytest.raises(nat.NativeError, match="solver must be 'gmres' or 'broyden'"):
        eng.implicit_grad64(batch, sd, ok, ok, solver="anderson", y=ok)
    for bad in (torch.zeros(7, 8), torch.zeros(6, 10)):
        with pytest.raises(nat.NativeError, match="h_star has shape"):
            eng.implicit_grad64(batch, sd, bad, ok)
        with pytest.raises(nat.NativeError, match="grad has shape"):
            eng.implicit_grad64(batch, sd, ok, bad)
        with pytest.raises(nat.NativeError, match="y has shape"):
            eng.implicit_grad64(batch, sd, ok, ok, y=bad)
    for w in (8, 16):   # a state dict of another latent width: forward inference only
        wide = {"deqdss.f.laynorm.weight": torch.zeros(w)}
        with pytest.raises(nat.NativeError, match="forward inference only"):
            eng.implicit_grad64(batch, wide, ok, ok)


def test_null_arguments_are_error_codes():
    nat = pkg("_native")
    lib = nat.lib()
    assert lib.psignn_f64_param_vjp(None, None, 1, None, None, None, None, None, None, None, None, None, 0, None) < 0
    assert "NULL" in lib.psignn_last_error().decode()
    assert lib.psignn_mlp2_f64_backward(None, None, 1, 4, 10, 10, None, None, None, None, None, None, 0, None) < 0
    assert "NULL" in lib.psignn_last_error().decode()
    assert lib.psignn_f64_param_vjp_workspace_doubles(None, 1) == -1
    assert lib.psignn_f64_param_vjp_workspace_doubles(1, 0) == -1   # n_layers < 1: refused before the handle is looked at
    assert lib.psignn_f64_param_vjp_chunk_rows() >= 1
    q = lib.psignn_mlp2_f64_backward_workspace_doubles
    assert q(0, 4, 10, 10) == 0 and q(1, 16, 16, 16) == q(128, 16, 16, 16) == 16 * 16 + 16 + 16 * 16 + 16
    assert q(129, 4, 10, 10) == 2 * (40 + 10 + 100 + 10)
    assert q(-1, 4, 10, 10) == -1 and q(5, 0, 10, 10) == -1 and q(5, 4, 17, 10) == -1 and q(5, 4, 10, 17) == -1
