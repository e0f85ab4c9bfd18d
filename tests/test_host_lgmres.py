"""CPU: augmented restarts (LGMRES) and the stall ratio of the float64 GMRES -- the restatement ``lgmres_ref.lgmres_adjoint`` on the
float64 oracle, the C ABI surface (``psignn_gmres64_create_aug``, ``psignn_gmres64_solve_*_opts``, ``psignn_newton64_create_aug``,
``psignn_newton64_solve_opts``), every refusal that needs no device, and the plan / ring arithmetic of csrc/gmres_dense.h on the
host (tests/host/lgmres_plan_check.cpp).

The runs of the restatement: ``AdjointProblem`` of tests/adjoint_gmres_ref.py, float64 oracle VJP, m = 10, eps 1e-10, budget 1500.
Counts on the host these lines were written on (they depend on H*, which comes from a chaotic fp32 Broyden solve on the CPU, so the
tests assert relations, not these numbers):

====================  ==============================  ==========================================================================
fixture               augment 0, stall 0.5            stall 1.0, augment 0 / 1 / 2: products (cycles, n_aug), error to truth()
====================  ==============================  ==========================================================================
hex13_dirichlet_s0    tolerance, 187, 6.9e-11         187 (18, 0) 4.5e-9 / 117 (12, 9) 2.1e-9 / 130 (13, 19) 4.2e-9
hex26_dirichlet_s0    stagnation, 55, lowest 2.2e-4   605 (56, 0) 4.8e-8 / 242 (23, 21) 1.4e-8 / 240 (23, 39) 7.0e-9
hex13_mixed_s1        stagnation, 44, lowest 6.9e-4   341 (32, 0) 9.9e-9 / 176 (17, 15) 8.1e-9 / 208 (20, 34) 1.7e-9
====================  ==============================  ==========================================================================

(The ratios augmented / plain are 0.40 - 0.70.)"""
import ctypes
import inspect
import os
import re
import shutil
import subprocess
import types

import pytest
import torch

import adjoint_gmres_ref as ref
import lgmres_ref as lg
import newton64_ref as nref
from conftest import ROOT, pkg

NEW = {"psignn_gmres64_create_aug": 4, "psignn_gmres64_solve_adjoint_opts": 19, "psignn_gmres64_solve_shifted_opts": 21,
       "psignn_newton64_create_aug": 4, "psignn_newton64_solve_opts": 21}
M, EPS, BUDGET = 10, 1e-10, 1500
_problems, _runs = {}, {}


def problem(name):
    if name not in _problems:
        _problems[name] = ref.AdjointProblem(name)
    return _problems[name]


def run(name, augment, stall):
    """One float64 run of the restatement, computed once and shared."""
    key = (name, augment, stall)
    if key not in _runs:
        p = problem(name)
        _runs[key] = lg.lgmres_adjoint(p.vjp64, p.grad.double(), EPS, BUDGET, m=M, augment=augment, stall=stall)
    return _runs[key]


def _same(a, b):
    assert torch.equal(a["result"], b["result"]) and a["result"].dtype == b["result"].dtype
    for k in ("nstep", "lowest", "rel_trace", "abs_trace", "n_cycles", "stop", "n_reorth"):
        assert a[k] == b[k], k


# ----------------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_defaults_are_gmres_adjoint_bit_for_bit(dtype):
    p = problem("hex13_dirichlet_s0")
    vjp, grad = (p.vjp32, p.grad) if dtype == torch.float32 else (p.vjp64, p.grad.double())
    for m, eps, budget in ((10, 1e-10, 1500), (50, 1e-6 if dtype == torch.float32 else 1e-11, 400)):
        want = ref.gmres_adjoint(vjp, grad, eps, budget, m=m)
        got = lg.lgmres_adjoint(vjp, grad, eps, budget, m=m, augment=0, stall=0.5)
        _same(got, want)
        assert got["n_aug"] == 0 and got["n_cycles"] >= 2


def test_defaults_of_the_linear_form_are_gmres_shifted_bit_for_bit():
    p = nref.LinearProblem("hex13_dirichlet_s0")
    for shift, transposed in ((1.0, True), (1.5, False)):
        want = nref.gmres_shifted(p.op(transposed), p.b, shift, 1e-8, 200, m=8)
        got = lg.lgmres_adjoint(p.op(transposed), p.b, 1e-8, 200, m=8, shift=shift, lin=True)
        _same(got, want)
        assert got["n_aug"] == 0 and got["n_cycles"] > 2


@pytest.mark.parametrize("name", ref.FIXTURES)
def test_the_halving_rule_is_what_stops_the_short_restart(name):
    plain, lifted = run(name, 0, 0.5), run(name, 0, 1.0)
    print(f"LGM {name}: stall 0.5 {plain['stop']} after {plain['nstep']} products, lowest {plain['lowest']:.3e}; stall 1.0 "
          f"{lifted['stop']} after {lifted['nstep']} products ({lifted['n_cycles']} cycles), lowest {lifted['lowest']:.3e}")
    if name in ("hex26_dirichlet_s0", "hex13_mixed_s1"):
        assert plain["stop"] == "stagnation" and plain["lowest"] > 1e-4
    assert lifted["stop"] == "tolerance" and lifted["lowest"] < EPS and lifted["n_aug"] == 0
    # the two runs are one run up to the cycle the halving rule ends
    n = plain["n_cycles"]
    assert lifted["rel_trace"][:n] == plain["rel_trace"]


@pytest.mark.parametrize("augment", [1, 2])
@pytest.mark.parametrize("name", ref.FIXTURES)
def test_kept_corrections_cut_the_products(name, augment):
    p = problem(name)
    base, got = run(name, 0, 1.0), run(name, augment, 1.0)
    e0, e1 = p.error(base["result"]), p.error(got["result"])
    print(f"LGM {name} augment {augment}: {got['stop']} after {got['nstep']} products ({got['n_cycles']} cycles, n_aug {got['n_aug']}, "
          f"n_reorth {got['n_reorth']}), lowest {got['lowest']:.3e}, error {e1:.2e}; augment 0: {base['nstep']} products, error {e0:.2e}; "
          f"ratio {got['nstep'] / base['nstep']:.2f}")
    assert base["stop"] == got["stop"] == "tolerance"
    assert got["nstep"] < base["nstep"]
    assert got["n_aug"] > 0 and got["n_aug"] <= augment * (got["n_cycles"] - 2)   # none in the first cycle, none after the last
    assert got["rel_trace"][0] == base["rel_trace"][0] and got["rel_trace"][1] == base["rel_trace"][1]   # the first cycle is plain
    assert e1 <= 4.0 * e0


def test_plan_of_the_restatement():
    for stored in range(0, 9):
        for augment in range(0, 9):
            for left in range(1, 13):
                nk, ka = lg.plan(stored, augment, left)
                assert nk >= 1 and nk + ka == left and 0 <= ka <= min(stored, augment)


# ----------------------------------------------------------------------------------------------------------------- the surface
def test_entries_in_header_table_and_default_library_only():
    nat = pkg("_native")
    hdr = open(os.path.join(ROOT, "include", "psignn_hip.h")).read()
    raw_hdr = hdr
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    decl = dict(re.findall(r"\b(psignn_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", hdr))
    lib = ctypes.CDLL(nat.LIB_PATH)
    rows = [l for l in open(os.path.join(ROOT, "INTEGRATION.md")).read().splitlines() if l.startswith("|")]
    for name, arity in NEW.items():
        assert name in decl, name
        assert decl[name].count(",") + 1 == arity, (name, decl[name])
        assert len(nat.SIGNATURES[name][1]) == arity, name
        assert hasattr(lib, name), name
        at = raw_hdr.index(name + "(", raw_hdr.index("psignn_gmres64_opts_t;"))
        before = raw_hdr[:at]
        assert "model.py:" in before[before.rindex("/*"):], name   # every entry cites its reference call site
        assert any(name in l and "model.py:" in l for l in rows), name
    for w in (8, 16):   # default-width library only
        raw = ctypes.CDLL(nat.lib_path(w))
        assert not any(hasattr(raw, n) for n in NEW), w
    # the structs the header declares are the ones ctypes passes
    assert [f[0] for f in nat.Gmres64Opts._fields_] == ["augment", "stall"] and ctypes.sizeof(nat.Gmres64Opts) == 16
    assert [f[0] for f in nat.Gmres64Info._fields_] == ["products", "cycles", "stop_reason", "n_reorth", "lowest", "lowest_abs", "n_aug"]
    assert [f[0] for f in nat.Gmres64Info._fields_][:6] == [f[0] for f in nat.GmresAdjointInfo._fields_]
    assert ctypes.sizeof(nat.Gmres64Info) == 40


def test_python_signatures():
    eng = pkg("engine")
    sig = lambda f: inspect.signature(f).parameters
    p = sig(eng.DeviceGmres64Aug.__init__)
    assert list(p) == ["self", "fmap64", "m", "augment"] and p["augment"].default == 0
    base = list(sig(eng.DeviceGmres64.solve_adjoint))
    p = sig(eng.DeviceGmres64Aug.solve_adjoint)
    assert list(p) == base + ["augment", "stall"] and (p["augment"].default, p["stall"].default) == (None, 0.5)
    base = list(sig(eng.DeviceGmres64.solve_shifted))
    p = sig(eng.DeviceGmres64Aug.solve_shifted)
    assert list(p) == base + ["augment", "stall"] and (p["augment"].default, p["stall"].default) == (None, 0.5)
    assert all(sig(eng.DeviceGmres64Aug.solve_shifted)[k].default == sig(eng.DeviceGmres64.solve_shifted)[k].default for k in base[3:])
    p = sig(eng.DeviceNewton64Aug.__init__)
    assert list(p) == ["self", "fmap64", "m", "augment"] and (p["m"].default, p["augment"].default) == (50, 0)
    base = list(sig(eng.DeviceNewton64.solve))
    p = sig(eng.DeviceNewton64Aug.solve)
    assert list(p) == base + ["lin_stall"] and p["lin_stall"].default == 0.5
    assert all(p[k].default == sig(eng.DeviceNewton64.solve)[k].default for k in base[2:])
    p = sig(eng.adjoint64_aug)
    assert list(p) == ["batch", "state_dict", "h_star", "grad", "eps", "m", "max_products", "augment", "stall"]
    assert [p[k].default for k in list(p)[4:]] == [1e-11, 50, 2000, 0, 0.5]
    assert issubclass(eng.DeviceGmres64Aug, eng.DeviceGmres64) and issubclass(eng.DeviceNewton64Aug, eng.DeviceNewton64)


def _hand_made_map(handle=1):
    """A map filled in by hand around a handle that is never used: the checks under test come before any native call."""
    eng = pkg("engine")
    fm = eng.FixedPointMap64.__new__(eng.FixedPointMap64)
    fm.plan = types.SimpleNamespace(mixed=False, N=7, E=20, device=torch.device("cpu"), handle=None)
    fm.weights = types.SimpleNamespace(width=10, n_layers=1, mixed=False)
    fm.handle, fm.device = handle, torch.device("cpu")
    return fm


def test_refusals_before_any_native_call():
    nat, eng = pkg("_native"), pkg("engine")
    fm = _hand_made_map()
    for cls in (eng.DeviceGmres64Aug, eng.DeviceNewton64Aug):
        for m, augment in ((5, 5), (5, -1), (20, 9), (1, 1)):   # augment >= m, negative, above 8
            with pytest.raises(nat.NativeError, match="augment must be in 0 .."):
                cls(fm, m, augment)
        with pytest.raises(nat.NativeError, match="open FixedPointMap64"):
            cls(_hand_made_map(handle=None), 5, 1)
    g = eng.DeviceGmres64Aug.__new__(eng.DeviceGmres64Aug)
    g.fmap, g.m, g.device, g.handle, g.augment = fm, 5, fm.device, 1, 2   # a handle made with two slots
    nt = eng.DeviceNewton64Aug.__new__(eng.DeviceNewton64Aug)
    nt.fmap, nt.m, nt.device, nt.handle, nt.augment = fm, 5, fm.device, 1, 2
    ok = torch.zeros(7, 10)
    for augment in (3, -1):
        with pytest.raises(nat.NativeError, match="augment must be in 0 .. 2"):
            g.solve_adjoint(ok, ok, 1e-11, 20, augment=augment)
        with pytest.raises(nat.NativeError, match="augment must be in 0 .. 2"):
            g.solve_shifted(ok, ok, augment=augment)
    for stall in (0.0, 1.5, float("nan"), -0.5, float("inf")):
        with pytest.raises(nat.NativeError, match=r"stall must be in \(0, 1\]"):
            g.solve_adjoint(ok, ok, 1e-11, 20, stall=stall)
        with pytest.raises(nat.NativeError, match=r"stall must be in \(0, 1\]"):
            g.solve_shifted(ok, ok, stall=stall)
        with pytest.raises(nat.NativeError, match=r"stall must be in \(0, 1\]"):
            nt.solve(ok, lin_stall=stall)
    # good options reach the checks of the plain solve: shapes, then the host tensors (there is no CPU route)
    with pytest.raises(nat.NativeError, match="h_star has shape"):
        g.solve_adjoint(torch.zeros(6, 10), ok, 1e-11, 20, augment=1, stall=1.0)
    with pytest.raises(nat.NativeError, match="device tensors"):
        g.solve_adjoint(ok, ok, 1e-11, 20, augment=1, stall=1.0)
    with pytest.raises(nat.NativeError, match="max_products"):
        g.solve_adjoint(ok, ok, 1e-11, 0, stall=1.0)
    g.handle = None
    with pytest.raises(nat.NativeError, match="closed"):
        g.solve_adjoint(ok, ok, 1e-11, 20)
    batch = types.SimpleNamespace(x=torch.zeros(7, 3))
    sd = {"deqdss.f.laynorm.weight": torch.zeros(10)}
    with pytest.raises(nat.NativeError, match="augment must be in 0 .."):
        eng.adjoint64_aug(batch, sd, ok, ok, m=4, augment=4)
    with pytest.raises(nat.NativeError, match=r"stall must be in \(0, 1\]"):
        eng.adjoint64_aug(batch, sd, ok, ok, stall=0.0)
    with pytest.raises(nat.NativeError, match="grad has shape"):
        eng.adjoint64_aug(batch, sd, ok, torch.zeros(7, 8))


def test_null_and_out_of_range_arguments_are_error_codes():
    nat = pkg("_native")
    lib = nat.lib()
    h = ctypes.c_void_p()
    for create in (lib.psignn_gmres64_create_aug, lib.psignn_newton64_create_aug):
        assert create(ctypes.byref(h), None, 5, 1) < 0 and not h.value
        assert "NULL" in lib.psignn_last_error().decode()
        assert create(None, None, 5, 1) < 0
    assert lib.psignn_gmres64_solve_adjoint_opts(None, None, 1, None, None, None, None, None, 1e-11, 10, 8, None, None, 0, None, None,
                                                 None, None, None) < 0
    assert "NULL" in lib.psignn_last_error().decode()
    assert lib.psignn_gmres64_solve_shifted_opts(None, None, 1, None, None, None, None, None, 1.0, 0, 1e-2, 10, 8, None, None, 0, None,
                                                 None, None, None, None) < 0
    assert "NULL" in lib.psignn_last_error().decode()
    assert lib.psignn_newton64_solve_opts(None, None, 1, None, None, None, None, None, None, None, 0, None, None, None, None, None, None,
                                          None, None, None, None) < 0
    assert "NULL" in lib.psignn_last_error().decode()


# ----------------------------------------------------------------------------------------------------------------- the inlines
def test_plan_and_ring_arithmetic_on_the_host(tmp_path):
    """tests/host/lgmres_plan_check.cpp includes only csrc/gmres_dense.h; compiled with the host compiler under AddressSanitizer
    and UBSan and run on its own."""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "lgmres_plan_check")
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *static,
                    "-I", os.path.join(ROOT, "psi-gnn_amd", "csrc"), os.path.join(ROOT, "tests", "host", "lgmres_plan_check.cpp"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "ok" and sum(l.startswith("case ") for l in lines) == 2
    assert "972 plans" in lines[0]   # 9 x 9 x 12
