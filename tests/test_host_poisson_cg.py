"""CPU: the device Poisson reference solve (``psignn_cg_*``, ``engine.PoissonCG``, ``compute_sol="device"``) -- its C ABI surface,
the argument checks that need no device, the Python signatures, and that the generator's existing values of ``compute_sol`` are
untouched."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, pkg

NEW = {"psignn_cg_create": 5, "psignn_cg_destroy": 1, "psignn_cg_solve": 11}


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
    assert "psignn_cg_t" in hdr and "psignn_cg_info_t" in hdr
    assert [f for f, _ in nat.CgInfo._fields_] == ["n_iter", "converged", "rel", "true_rel", "b_norm", "sym_defect"]
    assert ctypes.sizeof(nat.CgInfo) == 40
    # the problem has no latent width: like the plan's builders the solve is in the default library only
    for w in (8, 16):
        raw = ctypes.CDLL(nat.lib_path(w))
        assert not any(hasattr(raw, n) for n in NEW), w


def test_every_entry_has_an_integration_row():
    rows = [l for l in open(os.path.join(ROOT, "INTEGRATION.md")).read().splitlines() if l.startswith("|")]
    for name in NEW:
        short = name.replace("psignn_cg", "")
        assert any(name in l or ("psignn_cg_create" in l and short in l) for l in rows), name
    row = next(l for l in rows if "psignn_cg_create" in l)
    assert "extract_data.py" in row and "_solve" in row


def test_null_arguments_are_error_codes():
    nat = pkg("_native")
    lib = nat.lib()
    out = ctypes.c_void_p()
    info = nat.CgInfo()
    assert lib.psignn_cg_create(None, None, None, 0, None) < 0
    assert lib.psignn_cg_create(ctypes.byref(out), None, None, 1, None) < 0 and not out.value
    assert "NULL" in lib.psignn_last_error().decode()
    assert lib.psignn_cg_solve(None, None, 1, None, 1e-10, 10, 50, None, ctypes.byref(info), None, None) < 0
    lib.psignn_cg_destroy(None)   # a no-op, like the other destroy entries


def test_python_signatures():
    eng, hm = pkg("engine"), pkg("data.hexmesh")
    assert list(inspect.signature(eng.PoissonCG.__init__).parameters) == ["self", "plan", "a_ij"]
    p = inspect.signature(eng.PoissonCG.solve).parameters
    assert list(p) == ["self", "y", "x0", "tol", "max_iter", "poll_every"]
    assert (p["x0"].default, p["tol"].default, p["max_iter"].default, p["poll_every"].default) == (None, 1e-10, None, 50)
    assert callable(eng.PoissonCG.close)
    p = inspect.signature(eng.poisson_solve).parameters
    assert list(p) == ["batch", "tol", "kw"] and p["tol"].default == 1e-10 and p["kw"].kind is inspect.Parameter.VAR_KEYWORD
    assert eng.default_cg_max_iter(547) == 1000 and eng.default_cg_max_iter(1_000_519) == 20 * 1001
    for fn in (hm.make_hex_problem, hm.make_from_triangulation):
        assert inspect.signature(fn).parameters["compute_sol"].default is True


def test_device_solution_needs_a_gpu(monkeypatch):
    nat, data = pkg("_native"), pkg("data")
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)   # a host without a GPU, wherever this runs
    with pytest.raises(nat.NativeError, match="GPU"):
        data.make_hex_problem(3, compute_sol="device")
    with pytest.raises(ValueError):
        data.make_hex_problem(3, compute_sol="gpu")


def test_host_solution_is_still_spsolve_exactly():
    from scipy.sparse.linalg import spsolve
    data, hm = pkg("data"), pkg("data.hexmesh")
    n = 3
    pos, tri, q, r = hm.hex_lattice(n, hm.HSIZE, 0.15, 0.0)
    ring = np.maximum(np.maximum(np.abs(q), np.abs(r)), np.abs(-q - r)) == n
    K, M = hm.p1_assemble(pos, tri)
    pf, pg = hm._problem_coeffs(0)
    xs, ys = pos[:, 0] / (n * hm.HSIZE), pos[:, 1] / (n * hm.HSIZE)
    A, rhs = hm._apply_dirichlet(K, M @ hm._f_expr(pf, xs, ys), ring, hm._g_expr(pg, xs, ys))
    want = torch.tensor(spsolve(A.tocsc(), rhs)[:, None], dtype=torch.float32)
    assert torch.equal(data.make_hex_problem(n).sol, want)
    assert torch.equal(data.make_hex_problem(n, compute_sol=True).sol, want)
    assert torch.equal(data.make_hex_problem(n, compute_sol=False).sol, torch.zeros_like(want))
