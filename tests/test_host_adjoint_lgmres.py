"""CPU: augmented restarts (LGMRES) and the stall ratio of the fp32 GMRES adjoint solve (csrc/krylov.hip ``k_lg_*``,
``engine.DeviceGmresAug``, model keys ``bw_gmres_augment`` / ``bw_gmres_stall``) -- the C ABI surface, every refusal that needs no
device, the model keys, and the fp32 restatement ``lgmres_ref.lgmres_adjoint`` on the float32 oracle VJP.

The runs of the restatement: ``AdjointProblem.vjp32`` of tests/adjoint_gmres_ref.py, fp32 vectors, m = 10, eps 1e-5, budget 800.
Products / stop on the host these lines were written on (they depend on H*, which comes from a chaotic fp32 Broyden solve on the
CPU, so the tests assert the stop reasons and relations, not these counts):

====================  ======================  ================  ====================  ====================
fixture               today (0, 0.5)          stall 1.0         augment 1, stall 1.0  augment 2, stall 1.0
====================  ======================  ================  ====================  ====================
hex13_dirichlet_s0    77 tolerance            77 tolerance      52 tolerance          55 tolerance
hex13_mixed_s1        44 stagnation 6.9e-4    132 tolerance     74 tolerance          87 tolerance
hex26_dirichlet_s0    55 stagnation 2.2e-4    165 tolerance     88 tolerance          99 tolerance
====================  ======================  ================  ====================  ====================
"""
import ctypes
import inspect
import os
import re

import pytest
import torch

import adjoint_gmres_ref as ref
import lgmres_ref as lg
from conftest import ROOT, pkg

EINVAL = -1   # PSIGNN_EINVAL
NEW = {"psignn_gmres_create_aug": 8, "psignn_gmres_solve_adjoint_opts": 18, "psignn_gmres_solve_adjoint_lin_opts": 15}
M, EPS, BUDGET = 10, 1e-5, 800
STOPS = {"hex13_dirichlet_s0": "tolerance", "hex13_mixed_s1": "stagnation", "hex26_dirichlet_s0": "stagnation"}   # of (0, 0.5)
_problems, _runs = {}, {}


def problem(name):
    if name not in _problems:
        _problems[name] = ref.AdjointProblem(name)
    return _problems[name]


def run(name, augment, stall):
    """One fp32 run of the restatement, computed once and shared."""
    key = (name, augment, stall)
    if key not in _runs:
        p = problem(name)
        _runs[key] = lg.lgmres_adjoint(p.vjp32, p.grad, EPS, BUDGET, m=M, augment=augment, stall=stall)
    return _runs[key]


# ----------------------------------------------------------------------------------------------------------------- the surface
def test_entries_in_header_table_and_default_library_only():
    nat = pkg("_native")
    raw_hdr = open(os.path.join(ROOT, "include", "psignn_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw_hdr, flags=re.S)
    decl = dict(re.findall(r"\b(psignn_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", hdr))
    lib = ctypes.CDLL(nat.LIB_PATH)
    rows = [l for l in open(os.path.join(ROOT, "INTEGRATION.md")).read().splitlines() if l.startswith("|")]
    for name, arity in NEW.items():
        assert name in decl, name
        assert decl[name].count(",") + 1 == arity, (name, decl[name])
        assert len(nat.SIGNATURES[name][1]) == arity, name
        assert hasattr(lib, name), name
        at = raw_hdr.index(name + "(", raw_hdr.index("psignn_gmres_opts_t;"))
        before = raw_hdr[:at]
        assert "model.py:210-223" in before[before.rindex("/*"):], name   # every entry cites its reference call site
        assert any(name in l and "model.py:210-223" in l for l in rows), name
    for struct in ("psignn_gmres_opts_t", "psignn_gmres_info_t"):
        at = raw_hdr.rindex("typedef struct", 0, raw_hdr.index("} " + struct + ";"))
        assert "model.py:210-223" in raw_hdr[raw_hdr.rindex("/*", 0, at):at], struct
    for w in (8, 16):   # default-width library only
        raw = ctypes.CDLL(nat.lib_path(w))
        assert not any(hasattr(raw, n) for n in NEW), w
    # the structs the header declares are the ones ctypes passes
    assert [f[0] for f in nat.GmresOpts._fields_] == ["augment", "stall"] and ctypes.sizeof(nat.GmresOpts) == 16
    assert [f[0] for f in nat.GmresInfo._fields_] == [f[0] for f in nat.GmresAdjointInfo._fields_] + ["n_aug"]
    assert ctypes.sizeof(nat.GmresInfo) == 40 and ctypes.sizeof(nat.GmresAdjointInfo) == 32
    assert nat.GmresInfo.n_aug.offset == 32 and nat.GmresOpts.stall.offset == 8


def test_python_signatures():
    eng = pkg("engine")
    sig = lambda f: inspect.signature(f).parameters
    p = sig(eng.DeviceGmresAug.__init__)
    assert list(p) == ["self", "n_elems", "device", "m_max", "augment", "shard_elems"]
    assert (p["augment"].default, p["shard_elems"].default) == (0, None)
    assert list(sig(eng.DeviceGmres.__init__)) == ["self", "n_elems", "device", "m_max", "shard_elems"]   # pinned, unchanged
    base = sig(eng.DeviceGmres.solve_adjoint)
    assert list(base) == ["self", "fmap", "h_star", "grad", "eps", "max_products", "lin", "poll_every"]
    p = sig(eng.DeviceGmresAug.solve_adjoint)
    assert list(p) == list(base) + ["augment", "stall"] and (p["augment"].default, p["stall"].default) == (None, 0.5)
    assert all(p[k].default == base[k].default for k in base)
    assert issubclass(eng.DeviceGmresAug, eng.DeviceGmres)
    # the float64 callers of gmres64_opts get the structure they always got
    o = eng.gmres64_opts(None, 0.75, 3, "x")
    assert type(o) is pkg("_native").Gmres64Opts and (o.augment, o.stall) == (3, 0.75)
    o = eng.gmres64_opts(1, 1.0, 3, "x", pkg("_native").GmresOpts)
    assert type(o) is pkg("_native").GmresOpts and (o.augment, o.stall) == (1, 1.0)


def test_create_aug_argument_errors_are_error_codes():
    """Every refusal of psignn_gmres_create_aug comes before anything is allocated: no device is needed."""
    nat = pkg("_native")
    lib = nat.lib()
    h = ctypes.c_void_p()
    fake = 4096   # a non-NULL pointer that is never dereferenced: the call is refused first
    bad = [
        (64, 64, 10, fake, 10, fake, 0, "augment out of range"),     # augment > m - 1
        (64, 64, 20, fake, 9, fake, 0, "augment out of range"),      # above 8
        (64, 64, 10, fake, -1, fake, 0, "augment out of range"),
        (64, 64, 10, fake, 2, None, 0, "d_ring"),                    # a ring is needed
        (64, 64, 10, fake, 0, fake, 0, "d_ring"),                    # and none with augment 0
        (64, 64, 10, fake, 2, fake, 63, "shard_elems"),              # below n_elems
        (64, 64, 10, None, 2, fake, 0, "bad arguments"),             # no basis
        (0, 64, 10, fake, 2, fake, 0, "bad arguments"),
        (64, 62, 10, fake, 2, fake, 0, "row pitch"),
    ]
    for n, ld, m, basis, augment, ring, shard, what in bad:
        h.value = 7
        assert lib.psignn_gmres_create_aug(ctypes.byref(h), n, ld, m, basis, augment, ring, shard) == EINVAL, what
        assert not h.value and what in lib.psignn_last_error().decode(), (what, lib.psignn_last_error().decode())
    assert lib.psignn_gmres_create_aug(None, 64, 64, 10, fake, 2, fake, 0) < 0
    # the options are looked at before anything else: a NULL handle or NULL options is an error code, not a crash
    for fn, n_args in ((lib.psignn_gmres_solve_adjoint_opts, 18), (lib.psignn_gmres_solve_adjoint_lin_opts, 15)):
        sig = nat.SIGNATURES[fn.__name__][1]
        args = [0 if t in (ctypes.c_int, ctypes.c_int64) else 0.0 if t is ctypes.c_double else None for t in sig]
        assert fn(*args) == EINVAL
        assert "NULL" in lib.psignn_last_error().decode()


def _hand_made(augment=2, m=5):
    """A DeviceGmresAug filled in by hand around a handle that is never used: the checks under test come before any native call."""
    eng = pkg("engine")
    g = eng.DeviceGmresAug.__new__(eng.DeviceGmresAug)
    g.M, g.m, g.device, g.handle, g.augment = 70, m, torch.device("cpu"), 1, augment
    return g


def test_refusals_before_any_native_call(monkeypatch):
    nat, eng = pkg("_native"), pkg("engine")
    monkeypatch.setattr(nat, "lib", lambda *a: (_ for _ in ()).throw(AssertionError("the library was touched")))
    for m, augment in ((5, 5), (5, -1), (20, 9), (1, 1)):   # augment >= m, negative, above 8
        with pytest.raises(nat.NativeError, match="augment must be in 0 .."):
            eng.DeviceGmresAug(70, torch.device("cpu"), m, augment)
        with pytest.raises(nat.NativeError, match="augment must be in 0 .."):
            eng.check_augment(augment, m, "x")
    assert [eng.check_augment(a, 10, "x") for a in (0, 1, 8)] == [0, 1, 8] and eng.check_augment(4, 5, "x") == 4
    with pytest.raises(nat.NativeError, match="shard_elems"):
        eng.DeviceGmresAug(70, torch.device("cpu"), 10, 2, shard_elems=69)
    g = _hand_made()
    ok = torch.zeros(7, 10)
    for augment in (3, -1):
        with pytest.raises(nat.NativeError, match="augment must be in 0 .. 2"):
            g.solve_adjoint(None, ok, ok, 1e-8, 20, augment=augment)
    for stall in (0.0, 1.5, float("nan"), -0.5, float("inf")):
        with pytest.raises(nat.NativeError, match=r"stall must be in \(0, 1\]"):
            g.solve_adjoint(None, ok, ok, 1e-8, 20, stall=stall)


# ----------------------------------------------------------------------------------------------------------------- the model keys
def test_check_bw_gmres_aug():
    eng, nat = pkg("engine"), pkg("_native")
    assert eng.check_bw_gmres_aug(None, None, "gmres", 50) == (0, 0.5)
    assert eng.check_bw_gmres_aug(8, 1, "gmres", 50) == (8, 1.0) and eng.check_bw_gmres_aug(1, 0.25, "gmres", 2) == (1, 0.25)
    for bad in (-1, 9, 1.0, "1", True):
        with pytest.raises(nat.NativeError, match=r"bw_gmres_augment must be an int in 0\.\.min\(bw_gmres_m - 1, 8\) = 8"):
            eng.check_bw_gmres_aug(bad, None, "gmres", 50)
    with pytest.raises(nat.NativeError, match=r"bw_gmres_augment must be an int in 0\.\.min\(bw_gmres_m - 1, 8\) = 3"):
        eng.check_bw_gmres_aug(4, None, "gmres", 4)
    for bad in (0.0, 0, 1.5, -0.5, float("nan"), float("inf"), "0.5", True):
        with pytest.raises(nat.NativeError, match=r"bw_gmres_stall must be a float in \(0, 1\]"):
            eng.check_bw_gmres_aug(None, bad, "gmres", 50)
    for solver in (None, "broyden"):
        with pytest.raises(nat.NativeError, match="bw_gmres_augment / bw_gmres_stall need bw_solver"):
            eng.check_bw_gmres_aug(1, None, solver, 50)


@pytest.mark.parametrize("module", ["model_psignn", "mixed"])
def test_model_config_keys(module):
    nat = pkg("_native")
    mk = lambda **kw: pkg(module).ModelDEQDSS(dict(latent_dim=10, n_layers=1, bw_thres=40, **kw))
    for net in (mk(), mk(bw_solver="gmres")):   # absent: not in config_deq, and the solve without options
        assert "bw_gmres_augment" not in net.config_deq and "bw_gmres_stall" not in net.config_deq
        assert net.deqdss._bw_gmres_opts() is None
    net = mk(bw_solver="gmres", bw_gmres_m=10, bw_gmres_augment=2)
    assert net.config_deq["bw_gmres_augment"] == 2 and "bw_gmres_stall" not in net.config_deq and net.deqdss._bw_gmres_opts() == (2, 0.5)
    net = mk(bw_solver="gmres", bw_gmres_stall=1.0)
    assert net.config_deq["bw_gmres_stall"] == 1.0 and "bw_gmres_augment" not in net.config_deq and net.deqdss._bw_gmres_opts() == (0, 1.0)
    net = mk(bw_solver="gmres", bw_gmres_augment=0, bw_gmres_stall=0.5)   # present at their defaults: today's route
    assert net.config_deq["bw_gmres_augment"] == 0 and net.config_deq["bw_gmres_stall"] == 0.5 and net.deqdss._bw_gmres_opts() is None
    # values
    for aug, m in ((-1, 10), (9, 40), (10, 10), (1.0, 10), (True, 10)):
        with pytest.raises(nat.NativeError, match="bw_gmres_augment must be an int in 0..min"):
            mk(bw_solver="gmres", bw_gmres_m=m, bw_gmres_augment=aug)
    for stall in (0.0, 1.01, float("nan"), "1"):
        with pytest.raises(nat.NativeError, match="bw_gmres_stall must be a float in"):
            mk(bw_solver="gmres", bw_gmres_stall=stall)
    # either key without bw_solver = "gmres": an error naming both keys and bw_solver
    for kw in (dict(bw_gmres_augment=1), dict(bw_gmres_stall=1.0), dict(bw_solver=None, bw_gmres_augment=0),
               dict(bw_gmres_m=10, bw_gmres_stall=0.5)):
        with pytest.raises(nat.NativeError) as e:
            mk(**kw)
        assert all(k in str(e.value) for k in ("bw_gmres_augment", "bw_gmres_stall", 'bw_solver = "gmres"')), str(e.value)
    # the lockstep GMRES takes no options: with a non-default key the replicas run one after the other, whatever bw_gmres_lockstep says
    import types
    tiled = types.SimpleNamespace(plan=types.SimpleNamespace(tiled=True, mixed=False), weights=types.SimpleNamespace(n_layers=1),
                                  can_linearize=lambda: True, lin_neumann="direct")
    base = dict(bw_solver="gmres", bw_gmres_m=10, bw_gmres_lockstep=True)
    assert mk(**base).deqdss.lockstep_applies([tiled, tiled]) is True
    assert mk(**base, bw_gmres_augment=0, bw_gmres_stall=0.5).deqdss.lockstep_applies([tiled, tiled]) is True
    for kw in (dict(bw_gmres_augment=1), dict(bw_gmres_stall=1.0), dict(bw_gmres_augment=2, bw_gmres_stall=0.75)):
        assert mk(**base, **kw).deqdss.lockstep_applies([tiled, tiled]) is False
        assert mk(**base, **kw).deqdss.lockstep_applies([object()]) is False   # (decided before the maps are looked at)


@pytest.mark.parametrize("d", [8, 16])
def test_other_widths_stay_forward_only_with_the_keys(d, monkeypatch):
    nat, eng = pkg("_native"), pkg("engine")
    net = pkg("model_psignn").ModelDEQDSS(dict(latent_dim=d, n_layers=1, bw_solver="gmres", bw_gmres_m=10, bw_gmres_augment=1,
                                               bw_gmres_stall=1.0))
    monkeypatch.setattr(nat, "lib", lambda *a: (_ for _ in ()).throw(AssertionError("the library was touched")))
    deq = net.deqdss
    for call in (lambda: net.train()(object()), lambda: deq.train_forward(torch.zeros(3, d), object()),
                 lambda: deq.implicit_backward(None, None, object(), torch.zeros(3, d)),
                 lambda: deq.train_forward_replicas([torch.zeros(3, d)], [object()])):
        with pytest.raises(nat.NativeError, match=f"latent_dim {d} has forward inference only"):
            call()
    import types
    fmap = types.SimpleNamespace(width=d, plan=None, weights=None)
    with pytest.raises(nat.NativeError, match=f"latent_dim {d} has forward inference only"):
        _hand_made().solve_adjoint(fmap, torch.zeros(7, d), torch.zeros(7, d), 1e-8, 20, augment=1, stall=1.0)


# ----------------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("name", ref.FIXTURES)
def test_fp32_defaults_are_gmres_adjoint_bit_for_bit(name):
    p = problem(name)
    want = ref.gmres_adjoint(p.vjp32, p.grad, EPS, BUDGET, m=M)
    got = run(name, 0, 0.5)
    assert got["result"].dtype == torch.float32 and torch.equal(got["result"], want["result"])
    for k in ("nstep", "lowest", "rel_trace", "abs_trace", "n_cycles", "stop", "n_reorth"):
        assert got[k] == want[k], k
    assert got["n_aug"] == 0


@pytest.mark.parametrize("name", ref.FIXTURES)
def test_fp32_stop_reasons_and_products(name):
    """Table A of the module docstring: the stop reasons, and fewer products with one kept correction on all three fixtures."""
    plain, lifted, one, two = run(name, 0, 0.5), run(name, 0, 1.0), run(name, 1, 1.0), run(name, 2, 1.0)
    print(f"ADJOINT_LGMRES_REF {name}: " + " | ".join(f"({a}, {s}) {o['nstep']} {o['stop']} lowest {o['lowest']:.2e} n_aug {o['n_aug']}"
                                                      for (a, s), o in (((0, 0.5), plain), ((0, 1.0), lifted), ((1, 1.0), one), ((2, 1.0), two))))
    assert plain["stop"] == STOPS[name]
    if STOPS[name] == "stagnation":
        assert plain["lowest"] > 1e-4
        n = plain["n_cycles"]   # the two runs are one run up to the cycle the halving rule ends
        assert lifted["rel_trace"][:n] == plain["rel_trace"] and lifted["n_cycles"] > n
    for o in (lifted, one, two):
        assert o["stop"] == "tolerance" and o["lowest"] < EPS
    assert one["nstep"] < lifted["nstep"] and two["nstep"] < lifted["nstep"]
    assert lifted["n_aug"] == 0
    for augment, o in ((1, one), (2, two)):
        assert 0 < o["n_aug"] <= augment * (o["n_cycles"] - 1)
        assert o["rel_trace"][:2] == lifted["rel_trace"][:2]   # the first cycle is plain
