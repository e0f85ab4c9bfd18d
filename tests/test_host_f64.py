"""CPU: the float64 forward path (``psignn_f64_*``, ``psignn_mlp2_f64``, ``psignn_broyden64_*`` and their engine handles) -- the C ABI
surface, the weight layout's length, and every refusal that needs no device."""
import ctypes
import inspect
import os
import re
import types

import pytest
import torch

from conftest import ROOT, load_weights, pkg

NEW = {"psignn_f64_weights_size": 2, "psignn_f64_create": 5, "psignn_f64_destroy": 1, "psignn_f64_forward": 9, "psignn_mlp2_f64": 11,
       "psignn_broyden64_create": 3, "psignn_broyden64_destroy": 1, "psignn_broyden64_bytes": 1, "psignn_broyden64_solve": 14}


def _state_dict(mixed, n_layers, width=10):
    net = pkg("mixed" if mixed else "model_psignn").ModelPSIGNN(dict(latent_dim=width, n_layers=n_layers))
    return {k: v.detach().clone() for k, v in net.state_dict().items()}


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
    assert "psignn_f64_t" in hdr and "psignn_broyden64_t" in hdr
    for w in (8, 16):   # default-width library only
        raw = ctypes.CDLL(nat.lib_path(w))
        assert not any(hasattr(raw, n) for n in NEW), w


def test_every_entry_has_an_integration_row():
    rows = [l for l in open(os.path.join(ROOT, "INTEGRATION.md")).read().splitlines() if l.startswith("|")]
    for name in NEW:
        assert any(name in l for l in rows), name


@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("n_layers", [1, 2])
def test_weights_size_is_the_packed_length(mixed, n_layers):
    nat, eng = pkg("_native"), pkg("engine")
    sd = _state_dict(mixed, n_layers)
    w = eng.PackedWeights64(sd)     # packs on the CPU
    assert w.flat.dtype == torch.float64 and w.flat.device.type == "cpu" and (w.mixed, w.n_layers) == (mixed, n_layers)
    assert nat.lib().psignn_f64_weights_size(int(mixed), n_layers) == w.flat.numel()
    p = 3 if mixed else 2
    assert w.flat.numel() == 20 + 30 + p + 1 + n_layers * (2 * 350 + 10 * (30 + p) + 120) + (350 + 10 * (22 + p) + 120 if mixed else 0)
    # state-dict order, nothing derived: the blocks are the tensors themselves, widened exactly
    F = "deqdss.f."
    shared = 51 + p
    assert torch.equal(w.flat[:10], sd[F + "laynorm.weight"].double())
    assert torch.equal(w.flat[20:20 + 30 + p], sd[F + "alpha.0.weight"].double().reshape(-1))
    assert torch.equal(w.flat[shared:shared + 230], sd[F + "phi_to_list.0.mlp.mlp.0.weight"].double().reshape(-1))
    assert torch.equal(w.flat[shared + 700:shared + 700 + 10 * (30 + p)], sd[F + "update_list.0.mlp.0.weight"].double().reshape(-1))
    if mixed:
        assert torch.equal(w.flat[-120 - 10 * (22 + p):-120], sd[F + "update_neumann.mlp.0.weight"].double().reshape(-1))
    assert nat.lib().psignn_f64_weights_size(0, 0) == -1


def test_shipped_checkpoints_pack():
    eng = pkg("engine")
    assert eng.PackedWeights64(load_weights("dirichlet")).flat.numel() == 1193
    assert eng.PackedWeights64(load_weights("mixed")).flat.numel() == 1924


@pytest.mark.parametrize("width", [8, 16])
def test_other_widths_are_refused(width):
    nat, eng = pkg("_native"), pkg("engine")
    with pytest.raises(nat.NativeError, match=f"latent_dim {width} has forward inference only"):
        eng.PackedWeights64(_state_dict(False, 1, width))


def _fake_plan(mixed, N=7, E=20):
    return types.SimpleNamespace(mixed=mixed, N=N, E=E, device=torch.device("cpu"), handle=None)


def test_family_and_shape_mismatches_are_refused_on_the_host():
    nat, eng = pkg("_native"), pkg("engine")
    wd, wm = eng.PackedWeights64(load_weights("dirichlet")), eng.PackedWeights64(load_weights("mixed"))
    N, E = 7, 20
    h0, ea, nrm = torch.zeros(N, 10), torch.zeros(E, 3), torch.zeros(N, 2)
    with pytest.raises(nat.NativeError, match="family"):
        eng.FixedPointMap64(_fake_plan(True), wd, h0, torch.zeros(N, 3), ea, nrm)
    with pytest.raises(nat.NativeError, match="family"):
        eng.FixedPointMap64(_fake_plan(False), wm, h0, torch.zeros(N, 2), ea)
    with pytest.raises(nat.NativeError, match="unit_normal_vector"):
        eng.FixedPointMap64(_fake_plan(True), wm, h0, torch.zeros(N, 3), ea)
    for bad in (dict(prb=torch.zeros(N, 3)), dict(h0=torch.zeros(N, 8)), dict(ea=torch.zeros(E - 1, 3)), dict(h0=torch.zeros(N + 1, 10))):
        a = dict(h0=h0, prb=torch.zeros(N, 2), ea=ea)
        a.update(bad)
        with pytest.raises(nat.NativeError, match="shape mismatch"):
            eng.FixedPointMap64(_fake_plan(False), wd, a["h0"], a["prb"], a["ea"])
    # shapes right, tensors on the host: there is no CPU route
    with pytest.raises(nat.NativeError, match="device tensors"):
        eng.FixedPointMap64(_fake_plan(False), wd, h0, torch.zeros(N, 2), ea)
    with pytest.raises(nat.NativeError):
        eng.mlp2_64(torch.zeros(4, 1), torch.zeros(10, 1), torch.zeros(10), torch.zeros(10, 10), torch.zeros(10))


def _hand_made(handle=1):
    """A map and a solver filled in by hand around handles that are never used: the checks under test come before any native call."""
    eng = pkg("engine")
    fm = eng.FixedPointMap64.__new__(eng.FixedPointMap64)
    fm.plan, fm.handle, fm.device = _fake_plan(False), handle, torch.device("cpu")
    sv = eng.DeviceBroyden64.__new__(eng.DeviceBroyden64)
    sv.fmap, sv.threshold, sv.handle, sv.device = fm, 5, handle, fm.device
    return fm, sv


def test_wrong_x0_shape_and_closed_handles():
    nat, eng = pkg("_native"), pkg("engine")
    fm, sv = _hand_made()
    for shape in ((7, 8), (6, 10), (70,)):
        with pytest.raises(nat.NativeError, match="x0 has shape"):
            sv.solve(torch.zeros(*shape), 1e-9)
        with pytest.raises(nat.NativeError, match="H has shape"):
            fm(torch.zeros(*shape))
    sv.handle = None
    with pytest.raises(nat.NativeError, match="closed"):
        sv.solve(torch.zeros(7, 10), 1e-9)
    fm, sv = _hand_made()
    fm.handle = None
    with pytest.raises(nat.NativeError, match="closed"):
        fm(torch.zeros(7, 10))
    with pytest.raises(nat.NativeError, match="closed"):
        sv.solve(torch.zeros(7, 10), 1e-9)
    with pytest.raises(nat.NativeError, match="open FixedPointMap64"):
        eng.DeviceBroyden64(fm, 10)


def test_null_arguments_are_error_codes():
    nat = pkg("_native")
    lib = nat.lib()
    out = ctypes.c_void_p()
    info = nat.SolveInfo()
    assert lib.psignn_f64_create(None, None, None, 0, None) < 0
    assert lib.psignn_f64_create(ctypes.byref(out), None, None, 1, None) < 0 and not out.value
    assert "NULL" in lib.psignn_last_error().decode()
    assert lib.psignn_f64_forward(None, None, 1, None, None, None, None, None, None) < 0
    assert lib.psignn_mlp2_f64(None, 4, 1, 10, 10, None, None, None, None, None, None) < 0
    assert lib.psignn_broyden64_create(ctypes.byref(out), None, 10) < 0 and not out.value
    assert lib.psignn_broyden64_solve(None, None, 1, None, None, None, None, 1e-9, 16, None, ctypes.byref(info), None, None, None) < 0
    assert lib.psignn_broyden64_bytes(None) == 0
    lib.psignn_f64_destroy(None)
    lib.psignn_broyden64_destroy(None)


def test_shared_definitions_live_in_one_header():
    """``W64``, ``struct psignn_f64`` and the fixed-order reductions of the float64 path are defined once, in csrc/f64_common.h, the
    node block of f_theta once, in csrc/f64_node.h, and every object file is rebuilt when either header changes: two translation
    units can never read the handle or the weights at different offsets, sum in different orders, or state the gate, the update
    and LayerNorm differently."""
    csrc = os.path.join(ROOT, "psi-gnn_amd", "csrc")
    texts = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h"))}
    for head in ("template <int P>\nstruct W64 {", "struct psignn_f64 {"):
        assert {f: t.count(head) for f, t in texts.items() if head in t} == {"f64_common.h": 1}, head
    make = open(os.path.join(csrc, "Makefile")).read()
    hdrs = re.search(r"^HDRS := (.*)$", make, re.M).group(1).split()
    assert "f64_common.h" in hdrs
    assert re.search(r"^%\.o: %\.hip \$\(HDRS\)$", make, re.M)
    for f, t in texts.items():
        if f.endswith(".hip"):
            assert not re.search(r"\w+_(wave|block|final)_sum\((const )?double", t), f
    assert len(re.findall(r"\w+_(?:wave|block|final)_sum\((?:const )?double", texts["f64_common.h"])) == 3
    users = sorted(f for f, t in texts.items() if '#include "f64_common.h"' in t)
    assert users == ["f64_node.h", "fgnn_f64.hip", "fgnn_f64_deriv.hip", "krylov_f64.hip", "poisson_cg.hip", "solver_f64.hip"]
    assert "k_f64_pgrad" in texts["fgnn_f64_deriv.hip"]
    # the node block -- gate, update MLP, LayerNorm -- is stated once, in csrc/f64_node.h, which the map and its derivatives include
    assert "f64_node.h" in hdrs
    assert sorted(f for f, t in texts.items() if '#include "f64_node.h"' in t) == ["fgnn_f64.hip", "fgnn_f64_deriv.hip"]
    f64_files = users + ["f64_common.h", "newton_f64.hip"]
    for stmt in ("1.0 / (1.0 + exp(", "sqrt(var + 1e-5)"):   # the gate's sigmoid, the LayerNorm statistic
        assert {f: texts[f].count(stmt) for f in f64_files if stmt in texts[f]} == {"f64_node.h": 1}, stmt
    assert not [f for f, t in texts.items() if "k_f64_layer<" in t]


def test_python_signatures():
    eng = pkg("engine")
    sig = lambda f: inspect.signature(f).parameters
    assert list(sig(eng.PackedWeights64.__init__))[:3] == ["self", "sd", "device"]
    assert list(sig(eng.FixedPointMap64.__init__)) == ["self", "plan", "weights64", "h_initial", "prb_data", "edge_attr", "normals"]
    assert sig(eng.FixedPointMap64.__init__)["normals"].default is None
    assert list(sig(eng.DeviceBroyden64.__init__)) == ["self", "fmap64", "threshold"]
    p = sig(eng.DeviceBroyden64.solve)
    assert list(p) == ["self", "x0", "eps", "poll_every"] and p["poll_every"].default == 16
    p = sig(eng.fixed_point64)
    assert list(p)[:4] == ["batch", "state_dict", "eps", "threshold"] and (p["eps"].default, p["threshold"].default) == (1e-11, 1000)
    assert callable(eng.mlp2_64)
