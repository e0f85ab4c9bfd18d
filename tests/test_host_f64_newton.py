"""CPU: the float64 Newton-Krylov solver (``psignn_gmres64_solve_shifted``, ``psignn_newton64_*``; ``engine.DeviceGmres64.solve_shifted``,
``DeviceNewton64``, ``fixed_point64(solver=...)``) -- the step policy over a table of cases, the C ABI surface, every refusal that
needs no device, and the restatement of the shifted solve against a dense solve."""
import ctypes
import inspect
import math
import os
import re
import types

import pytest
import torch

from conftest import ROOT, load_weights, pkg

NEW = {"psignn_gmres64_solve_shifted": 20, "psignn_newton64_policy": 7, "psignn_newton64_create": 3, "psignn_newton64_destroy": 1,
       "psignn_newton64_bytes": 1, "psignn_newton64_solve": 20}
NAN, INF = float("nan"), float("inf")

# (sigma, g_old, g_new, growth, reject_floor, sigma_off) -> (accepted, next sigma)
POLICY = [
    # accepted: switched evolution relaxation, sigma * g_new / g_old
    ((1.0, 2.0, 1.0, 2.0, 0.0625, 1e-8), (True, 0.5)),
    ((0.5, 1.0, 1.5, 2.0, 0.0625, 1e-8), (True, 0.75)),          # |g| may grow up to `growth` times
    ((0.5, 1.0, 2.0, 2.0, 0.0625, 1e-8), (True, 1.0)),           # g_new == growth * g_old is not a rejection
    ((0.3, 7.0, 0.7, 2.0, 0.0625, 1e-8), (True, 0.3 * 0.7 / 7.0)),
    # a result below sigma_off is exactly 0
    ((1e-6, 1.0, 1e-3, 2.0, 0.0625, 1e-8), (True, 0.0)),
    ((1e-6, 1.0, 1e-2, 2.0, 0.0625, 1e-8), (True, 1e-6 * 1e-2 / 1.0)),   # exactly sigma_off stays
    ((1.0, 1.0, 0.5, 2.0, 0.0625, 0.75), (True, 0.0)),
    # sigma = 0 stays 0 on an accepted step
    ((0.0, 1.0, 0.5, 2.0, 0.0625, 1e-8), (True, 0.0)),
    ((0.0, 1.0, 1.9, 2.0, 0.0625, 1e-8), (True, 0.0)),
    ((0.0, 1.0, 0.0, 2.0, 0.0625, 1e-8), (True, 0.0)),
    # rejected on growth: max(4 sigma, reject_floor)
    ((0.5, 1.0, 2.0000001, 2.0, 0.0625, 1e-8), (False, 2.0)),
    ((1.0, 1.0, 0.5, 1e-3, 0.0625, 1e-8), (False, 4.0)),
    ((0.0, 1.0, 3.0, 2.0, 0.0625, 1e-8), (False, 0.0625)),       # from sigma = 0: the floor
    ((0.01, 1.0, 3.0, 2.0, 0.0625, 1e-8), (False, 0.0625)),      # 4 sigma below the floor: the floor
    ((0.015625, 1.0, 3.0, 2.0, 0.0625, 1e-8), (False, 0.0625)),  # 4 sigma == floor
    ((0.02, 1.0, 3.0, 2.0, 0.0625, 1e-8), (False, 0.08)),        # sigma > floor / 4: 4 sigma
    ((0.0625, 1.0, 3.0, 2.0, 0.0625, 1e-8), (False, 0.25)),
    ((0.25, 1.0, 3.0, 2.0, 0.0625, 1e-8), (False, 1.0)),
    # rejected on a value that is not finite
    ((0.5, 1.0, NAN, 2.0, 0.0625, 1e-8), (False, 2.0)),
    ((0.5, 1.0, INF, 2.0, 0.0625, 1e-8), (False, 2.0)),
    ((0.0, 1.0, NAN, 2.0, 0.0625, 1e-8), (False, 0.0625)),
    ((0.0, 1.0, INF, 1e30, 0.5, 1e-8), (False, 0.5)),
]


@pytest.mark.parametrize("args,want", POLICY)
def test_policy(args, want):
    nat, eng = pkg("_native"), pkg("engine")
    acc = ctypes.c_int(-1)
    nxt = nat.lib().psignn_newton64_policy(*args, ctypes.byref(acc))
    assert (bool(acc.value), nxt) == want and acc.value in (0, 1)
    assert nat.lib().psignn_newton64_policy(*args, None) == nxt   # the flag is optional
    sig, g_old, g_new, growth, floor, off = args
    assert eng.newton64_policy(sig, g_old, g_new, growth=growth, reject_floor=floor, sigma_off=off) == want


def test_policy_defaults_and_the_reject_ladder():
    eng = pkg("engine")
    d = inspect.signature(eng.newton64_policy).parameters
    assert (d["growth"].default, d["reject_floor"].default, d["sigma_off"].default) == (2.0, 0.0625, 1e-8)
    sigma, ladder = 0.0, []
    for _ in range(3):
        acc, sigma = eng.newton64_policy(sigma, 1.0, 10.0)
        assert not acc
        ladder.append(sigma)
    assert ladder == [0.0625, 0.25, 1.0]
    # SER down to plain Newton: a constant contraction of 0.1 from sigma = 1 reaches exactly 0 after the step that goes below 1e-8
    sigma, g, steps = 1.0, 1.0, 0
    while sigma > 0.0:
        acc, sigma = eng.newton64_policy(sigma, g, 0.1 * g)
        g, steps = 0.1 * g, steps + 1
        assert acc and steps < 20
    assert steps == 9 and sigma == 0.0


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
    assert "psignn_newton64_opts_t" in hdr and "psignn_newton64_info_t" in hdr
    assert [f for f, _ in nat.Newton64Opts._fields_] == ["eps", "sigma0", "eta", "growth", "reject_floor", "sigma_off", "threshold",
                                                         "max_products", "max_rejects", "poll_every"]
    assert [f for f, _ in nat.Newton64Info._fields_] == ["nstep", "n_iter", "n_accepted", "n_products", "n_feval", "stop_reason",
                                                         "lowest", "lowest_abs"]
    assert ctypes.sizeof(nat.Newton64Opts) == 64 and ctypes.sizeof(nat.Newton64Info) == 40
    for i, name in enumerate(pkg("engine").NEWTON_STOPS):
        assert re.search(rf"#define PSIGNN_NEWTON_{name.upper()} {i}\b", hdr), name


def test_every_entry_cites_the_forward_solve():
    """Each new declaration's comment in the header and each row of INTEGRATION.md names the call site it replaces, the forward
    solve of DeepEquilibrium.forward, dirichlet/psignn/model.py:189."""
    hdr = open(os.path.join(ROOT, "include", "psignn_hip.h")).read()
    rows = [l for l in open(os.path.join(ROOT, "INTEGRATION.md")).read().splitlines() if l.startswith("|")]
    for name in NEW:
        at = hdr.index(name + "(")
        before = hdr[:at]
        comment = before[before.rindex("/*"):] + hdr[at:hdr.index("\n", hdr.index(";", at))]
        assert "model.py:189" in comment, name
        hits = [l for l in rows if name in l]
        assert hits and any("model.py:189" in l for l in hits), name


def test_makefile_builds_the_unit_into_the_default_library_only():
    mk = open(os.path.join(ROOT, "psi-gnn_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", mk, flags=re.M).group(1).split()
    fwd = re.search(r"^FWD_SRCS := (.*)$", mk, flags=re.M).group(1).split()
    assert "newton_f64.hip" in srcs and "newton_f64.hip" not in fwd


def test_python_signatures():
    eng = pkg("engine")
    sig = lambda f: inspect.signature(f).parameters
    p = sig(eng.DeviceGmres64.solve_shifted)
    assert list(p) == ["self", "h", "b", "shift", "transposed", "eta", "max_products", "poll_every"]
    assert [p[k].default for k in list(p)[3:]] == [1.0, False, 1e-2, 200, 8]
    p = sig(eng.DeviceNewton64.__init__)
    assert list(p) == ["self", "fmap64", "m"] and p["m"].default == 50
    p = sig(eng.DeviceNewton64.solve)
    assert list(p) == ["self", "x0", "eps", "threshold", "sigma0", "eta", "max_products", "growth", "reject_floor", "sigma_off",
                       "max_rejects", "poll_every"]
    assert [p[k].default for k in list(p)[2:]] == [1e-11, 50, 1.0, 1e-2, 200, 2.0, 0.0625, 1e-8, 8, 8]
    assert isinstance(eng.DeviceNewton64.nbytes, property) and callable(eng.DeviceNewton64.close)
    p = sig(eng.fixed_point64)
    assert list(p) == ["batch", "state_dict", "eps", "threshold", "poll_every", "solver", "solver_kwargs"]
    assert p["solver"].default == "broyden" and p["solver_kwargs"].kind is inspect.Parameter.VAR_KEYWORD
    assert "not tuned on a GPU" in eng.DeviceNewton64.__doc__


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
    g = eng.DeviceGmres64.__new__(eng.DeviceGmres64)
    g.fmap, g.m, g.device, g.handle = fm, 5, fm.device, 1
    n = eng.DeviceNewton64.__new__(eng.DeviceNewton64)
    n.fmap, n.m, n.device, n.handle = fm, 5, fm.device, 1
    return g, n


def test_refusals_before_any_native_call():
    nat, eng = pkg("_native"), pkg("engine")
    fm = _hand_made_map()
    g, n = _hand_made_solvers(fm)
    ok = torch.zeros(7, 10)
    for shape in ((7, 8), (6, 10), (70,)):
        bad = torch.zeros(*shape)
        with pytest.raises(nat.NativeError, match="h has shape"):
            g.solve_shifted(bad, ok)
        with pytest.raises(nat.NativeError, match="b has shape"):
            g.solve_shifted(ok, bad)
        with pytest.raises(nat.NativeError, match="x0 has shape"):
            n.solve(bad)
    with pytest.raises(nat.NativeError, match="device tensors"):   # shapes right, tensors on the host: there is no CPU route
        g.solve_shifted(ok, ok)
    with pytest.raises(nat.NativeError, match="device tensors"):
        n.solve(ok)
    for s in (0.999, 0.0, -2.0, NAN, INF):
        with pytest.raises(nat.NativeError, match="shift must be finite and >= 1"):
            g.solve_shifted(ok, ok, shift=s)
    for v in (NAN, INF, -INF, -1e-9):
        with pytest.raises(nat.NativeError, match="eta must be"):
            g.solve_shifted(ok, ok, eta=v)
        with pytest.raises(nat.NativeError, match="eta must be"):
            n.solve(ok, eta=v)
        with pytest.raises(nat.NativeError, match="eps must be"):
            n.solve(ok, eps=v)
        with pytest.raises(nat.NativeError, match="sigma0 must be"):
            n.solve(ok, sigma0=v)
    with pytest.raises(nat.NativeError, match="max_products"):
        g.solve_shifted(ok, ok, max_products=0)
    for k in ("threshold", "max_products", "max_rejects"):
        with pytest.raises(nat.NativeError, match=k):
            n.solve(ok, **{k: 0})
    for k in ("growth", "reject_floor"):
        with pytest.raises(nat.NativeError, match=k):
            n.solve(ok, **{k: 0.0})
    for w in (8, 16):
        wg, wn = _hand_made_solvers(_hand_made_map(width=w))
        with pytest.raises(nat.NativeError, match="forward inference only"):
            wg.solve_shifted(ok, ok)
        with pytest.raises(nat.NativeError, match="forward inference only"):
            wn.solve(ok)
        with pytest.raises(nat.NativeError, match="forward inference only"):
            eng.DeviceNewton64(_hand_made_map(width=w))
    fm.handle = None   # the map is closed
    for call in (lambda: g.solve_shifted(ok, ok), lambda: n.solve(ok)):
        with pytest.raises(nat.NativeError, match="closed"):
            call()
    fm.handle = 1
    g.handle = n.handle = None   # the solvers are
    for call in (lambda: g.solve_shifted(ok, ok), lambda: n.solve(ok)):
        with pytest.raises(nat.NativeError, match="closed"):
            call()
    with pytest.raises(nat.NativeError, match="open FixedPointMap64"):
        eng.DeviceNewton64(_hand_made_map(handle=None))


def test_fixed_point64_refusals():
    nat, eng = pkg("_native"), pkg("engine")
    sd = load_weights("dirichlet")
    batch = types.SimpleNamespace(x=torch.zeros(7, 3))
    with pytest.raises(nat.NativeError, match="solver must be 'broyden' or 'newton'"):
        eng.fixed_point64(batch, sd, solver="anderson")
    with pytest.raises(nat.NativeError, match="takes no further keywords"):
        eng.fixed_point64(batch, sd, sigma0=0.0)


def test_null_arguments_are_error_codes():
    nat = pkg("_native")
    lib = nat.lib()
    assert lib.psignn_gmres64_solve_shifted(None, None, 1, None, None, None, None, None, 1.5, 0, 1e-2, 10, 8, None, 0, None, None, None,
                                            None, None) < 0
    assert "NULL" in lib.psignn_last_error().decode()
    assert lib.psignn_newton64_solve(None, None, 1, None, None, None, None, None, None, 0, None, None, None, None, None, None, None,
                                     None, None, None) < 0
    assert "NULL" in lib.psignn_last_error().decode()
    h = ctypes.c_void_p()
    assert lib.psignn_newton64_create(ctypes.byref(h), None, 5) < 0 and not h.value
    assert "NULL" in lib.psignn_last_error().decode()
    assert lib.psignn_newton64_create(None, None, 5) < 0
    assert lib.psignn_newton64_bytes(None) == 0
    lib.psignn_newton64_destroy(None)


@pytest.mark.parametrize("shift", [1.0, 1.5])
def test_restatement_against_a_dense_solve(shift):
    """``newton64_ref.gmres_shifted`` on a random contraction: the answer of ``(shift I - A) d = b``, the linear measure in the
    trace, the stop reasons, and the zero right-hand side."""
    import newton64_ref as ref
    gen = torch.Generator().manual_seed(3)
    n = 40
    A = torch.randn(n, n, generator=gen, dtype=torch.float64)
    A *= 0.7 / float(torch.linalg.matrix_norm(A, 2))
    b = torch.randn(n, generator=gen, dtype=torch.float64)
    want = torch.linalg.solve(shift * torch.eye(n, dtype=torch.float64) - A, b)
    op = lambda v: A @ v
    out = ref.gmres_shifted(op, b, shift, 1e-12, 400, m=15)
    assert out["stop"] == "tolerance" and out["lowest"] <= 1e-12 and out["n_cycles"] > 2
    assert float((out["result"] - want).norm() / want.norm()) <= 1e-11
    res = float((shift * out["result"] - A @ out["result"] - b).norm() / b.norm())
    assert math.isclose(res, out["lowest"], rel_tol=1e-3) and out["rel_trace"][0] == 1.0
    loose = ref.gmres_shifted(op, b, shift, 1e-2, 400, m=15)
    assert loose["stop"] == "tolerance" and 1e-4 < loose["lowest"] <= 1e-2 and loose["nstep"] < out["nstep"]
    assert ref.gmres_shifted(op, b, shift, 1e-12, 7, m=15)["stop"] == "budget"
    zero = ref.gmres_shifted(op, torch.zeros_like(b), shift, 1e-2, 400, m=15)
    assert (zero["nstep"], zero["n_cycles"], zero["stop"], zero["lowest"]) == (0, 1, "tolerance", 0.0) and not bool(zero["result"].any())
