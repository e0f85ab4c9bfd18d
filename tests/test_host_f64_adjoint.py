"""CPU: the float64 adjoint solves (``psignn_broyden64_solve_adjoint``, ``psignn_gmres64_*``; ``engine.DeviceBroyden64.solve_adjoint``,
``DeviceGmres64``, ``adjoint64``) -- the C ABI surface, every refusal that needs no device, and the dense part of the GMRES
(csrc/gmres_dense.h) against a least-squares solve on the host."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess
import types

import pytest
import torch

from conftest import ROOT, load_weights, pkg

NEW = {"psignn_broyden64_solve_adjoint": 17, "psignn_gmres64_create": 3, "psignn_gmres64_destroy": 1, "psignn_gmres64_bytes": 1,
       "psignn_gmres64_solve_adjoint": 18}


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


def test_every_entry_cites_the_backward_hook():
    """Each new declaration's comment in the header and each row of INTEGRATION.md names dirichlet/psignn/model.py:210-223."""
    hdr = open(os.path.join(ROOT, "include", "psignn_hip.h")).read()
    rows = [l for l in open(os.path.join(ROOT, "INTEGRATION.md")).read().splitlines() if l.startswith("|")]
    for name in NEW:
        at = hdr.index(name + "(")
        before = hdr[:at]
        comment = before[before.rindex("/*"):] + hdr[at:hdr.index("\n", hdr.index(";", at))]
        assert "model.py:210-223" in comment, name
        hits = [l for l in rows if name in l]
        assert hits and any("model.py:210-223" in l for l in hits), name


def test_makefile_builds_the_unit_into_the_default_library_only():
    mk = open(os.path.join(ROOT, "psi-gnn_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", mk, flags=re.M).group(1).split()
    fwd = re.search(r"^FWD_SRCS := (.*)$", mk, flags=re.M).group(1).split()
    assert "krylov_f64.hip" in srcs and "krylov_f64.hip" not in fwd
    assert "gmres_dense.h" in re.search(r"^HDRS := (.*)$", mk, flags=re.M).group(1).split()


def test_python_signatures():
    eng = pkg("engine")
    sig = lambda f: inspect.signature(f).parameters
    p = sig(eng.DeviceBroyden64.solve_adjoint)
    assert list(p) == ["self", "h_star", "grad", "eps", "poll_every"] and p["poll_every"].default == 16
    assert list(sig(eng.DeviceGmres64.__init__)) == ["self", "fmap64", "m"]
    p = sig(eng.DeviceGmres64.solve_adjoint)
    assert list(p) == ["self", "h_star", "grad", "eps", "max_products", "poll_every"] and p["poll_every"].default == 8
    assert isinstance(eng.DeviceGmres64.nbytes, property) and callable(eng.DeviceGmres64.close)
    p = sig(eng.adjoint64)
    assert list(p) == ["batch", "state_dict", "h_star", "grad", "solver", "eps", "m", "max_products", "threshold"]
    assert [p[k].default for k in ("solver", "eps", "m", "max_products", "threshold")] == ["gmres", 1e-11, 50, 2000, 800]


def _hand_made_map(handle=1, width=10):
    """A map filled in by hand around a handle that is never used: the checks under test come before any native call."""
    eng = pkg("engine")
    fm = eng.FixedPointMap64.__new__(eng.FixedPointMap64)
    fm.plan = types.SimpleNamespace(mixed=False, N=7, E=20, device=torch.device("cpu"), handle=None)
    fm.weights = types.SimpleNamespace(width=width, n_layers=1, mixed=False)
    fm.handle, fm.device = handle, torch.device("cpu")
    return fm


def _hand_made_solvers(fm):
    eng = pkg("engine")
    b = eng.DeviceBroyden64.__new__(eng.DeviceBroyden64)
    b.fmap, b.threshold, b.device, b.handle = fm, 5, fm.device, 1
    g = eng.DeviceGmres64.__new__(eng.DeviceGmres64)
    g.fmap, g.m, g.device, g.handle = fm, 5, fm.device, 1
    return [lambda h, y: b.solve_adjoint(h, y, 1e-11), lambda h, y: g.solve_adjoint(h, y, 1e-11, 20)], (b, g)


def test_wrong_shapes_closed_handles_and_other_widths():
    nat = pkg("_native")
    fm = _hand_made_map()
    calls, (b, g) = _hand_made_solvers(fm)
    ok = torch.zeros(7, 10)
    for call in calls:
        for shape in ((7, 8), (6, 10), (70,)):
            bad = torch.zeros(*shape)
            with pytest.raises(nat.NativeError, match="h_star has shape"):
                call(bad, ok)
            with pytest.raises(nat.NativeError, match="grad has shape"):
                call(ok, bad)
        with pytest.raises(nat.NativeError, match="device tensors"):   # shapes right, tensors on the host: there is no CPU route
            call(ok, ok)
    with pytest.raises(nat.NativeError, match="max_products"):
        g.solve_adjoint(ok, ok, 1e-11, 0)
    for w in (8, 16):
        wcalls, _ = _hand_made_solvers(_hand_made_map(width=w))
        for call in wcalls:
            with pytest.raises(nat.NativeError, match="forward inference only"):
                call(ok, ok)
    fm.handle = None   # the map is closed
    for call in calls:
        with pytest.raises(nat.NativeError, match="closed"):
            call(ok, ok)
    fm.handle = 1
    b.handle = g.handle = None   # the solvers are
    for call in calls:
        with pytest.raises(nat.NativeError, match="closed"):
            call(ok, ok)
    eng = pkg("engine")
    closed = _hand_made_map(handle=None)
    with pytest.raises(nat.NativeError, match="open FixedPointMap64"):
        eng.DeviceGmres64(closed, 5)


def test_adjoint64_refusals():
    nat, eng = pkg("_native"), pkg("engine")
    sd = load_weights("dirichlet")
    batch = types.SimpleNamespace(x=torch.zeros(7, 3))
    ok = torch.zeros(7, 10)
    with pytest.raises(nat.NativeError, match="solver must be"):
        eng.adjoint64(batch, sd, ok, ok, solver="anderson")
    with pytest.raises(nat.NativeError, match="h_star has shape"):
        eng.adjoint64(batch, sd, torch.zeros(6, 10), ok)
    with pytest.raises(nat.NativeError, match="grad has shape"):
        eng.adjoint64(batch, sd, ok, torch.zeros(7, 8), solver="broyden")
    for w in (8, 16):
        with pytest.raises(nat.NativeError, match="forward inference only"):
            eng.adjoint64(batch, {"deqdss.f.laynorm.weight": torch.zeros(w)}, ok, ok)


def test_null_arguments_are_error_codes():
    nat = pkg("_native")
    lib = nat.lib()
    assert lib.psignn_broyden64_solve_adjoint(None, None, 1, None, None, None, None, None, 1e-11, 16, None, 0, None, None, None, None,
                                              None) < 0
    assert "NULL" in lib.psignn_last_error().decode()
    assert lib.psignn_gmres64_solve_adjoint(None, None, 1, None, None, None, None, None, 1e-11, 10, 8, None, 0, None, None, None, None,
                                            None) < 0
    assert "NULL" in lib.psignn_last_error().decode()
    h = ctypes.c_void_p()
    assert lib.psignn_gmres64_create(ctypes.byref(h), None, 5) < 0 and not h.value
    assert "NULL" in lib.psignn_last_error().decode()
    assert lib.psignn_gmres64_create(None, None, 5) < 0
    assert lib.psignn_gmres64_bytes(None) == 0
    lib.psignn_gmres64_destroy(None)


def test_dense_part_against_least_squares(tmp_path):
    """tests/host/gmres_dense_check.cpp includes only csrc/gmres_dense.h; compiled with the host compiler under AddressSanitizer
    and UBSan and run on its own."""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "gmres_dense_check")
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *static,
                    "-I", os.path.join(ROOT, "psi-gnn_amd", "csrc"), os.path.join(ROOT, "tests", "host", "gmres_dense_check.cpp"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "ok" and sum(l.startswith("case ") for l in lines) == 48
