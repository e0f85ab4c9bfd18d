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


# ------------------------------------------------------------------------------------------------ the reference pieces of
# tests/test_gpu_poisson_cg_structure.py, held to that file's own gates without a device
import poisson_cg_ref as ref

TOL = 1e-12


@pytest.mark.parametrize("name", ref.STRUCTURE_CASES)
def test_numpy_recurrences_meet_the_gate_of_the_device_test(name):
    """|x - u|_F / |u|_F <= kappa_gershgorin true_rel against lifted_direct, for pcg_trace at the device test's tol."""
    _, A, y, dmask, u, kappa = ref.structure_case(name)
    x, trace = ref.pcg_trace(A, y, dmask, TOL, 1000)
    true_rel = ref.true_rel_of(A, y, dmask, x)
    err, lim = ref.gate(x, u, dmask, kappa, true_rel)
    print(f"{name}: iterations {len(trace) - 1} true_rel {true_rel:.3e} err {err:.3e} bound {lim:.3e} (kappa <= {kappa:.2f})")
    assert trace[-1] <= TOL and true_rel <= 10 * TOL
    assert err <= lim and kappa <= 9.0 * (1 + 1e-6)   # float32 rounding of the hub's diagonal moves rho = 0.8 by 1e-7
    assert np.array_equal(x[dmask], y[dmask])


def test_structure_cases_reach_the_paths_they_are_named_for():
    depth = lambda A, dmask, s: int((np.diff(A.indptr)[64 * s:64 * s + 64] * ~dmask[64 * s:64 * s + 64]).max())
    _, A, _, dmask = ref.structure_case("hub321")[:4]
    lens = np.diff(A.indptr)
    assert A.shape[0] == 321 and lens[0] == 321 and not dmask[0] and set(lens[1:]) == {3, 4}
    assert [depth(A, dmask, s) for s in range(6)] == [321, 0, 4, 4, 4, 3]           # a deep lane, a depth-0 slice, a one-row tail slice
    assert dmask[64:128].all() and dmask[300:].sum() == 3 and not dmask[320]
    _, A, _, dmask = ref.structure_case("lonely")[:4]
    lens, free = np.diff(A.indptr), ~dmask
    assert A.shape[0] == 130 and (lens[free] == 1).sum() == 6                       # free rows that hold their diagonal only
    assert np.flatnonzero(free[64:128]).tolist() == [63] and np.flatnonzero(free[128:]).tolist() == [0]
    rows = ref.one_by_one_rows(A, dmask)
    assert [int(i) for i in rows] == [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 63, 127, 128] and free.sum() - len(rows) == 48
    assert sorted(set(lens[free])) == [1, 2, 3, 4]
    for N, nblk, n_slices in ((65536, 256, 1024), (65537, 257, 1025)):
        mesh, A, _, dmask = ref.structure_case(f"band{N}")[:4]
        r, c = mesh.edge_index.numpy()
        assert A.shape[0] == N and -(-N // 256) == nblk and -(-N // 64) == n_slices
        assert np.abs(r - c).max() == 11 and 0.09 < dmask.mean() < 0.11
        assert len({depth(A, dmask, s) for s in range(n_slices)}) > 3


def test_lifted_direct_solves_the_free_rows_and_direct_does_not():
    _, A, y, dmask, u, _ = ref.structure_case("hub321")
    F = ~dmask
    assert np.array_equal(u[dmask], y[dmask])
    assert np.linalg.norm((A @ u - y)[F]) <= 1e-13 * np.linalg.norm(y[F])
    w = ref.direct(A, y)                                   # solves the Dirichlet rows too: another system
    assert np.linalg.norm((w - u)[F]) > 1e-3 * np.linalg.norm(u[F])


@pytest.mark.parametrize("name", ["hub321", "hub321_f32", "lonely"])
def test_gershgorin_bounds_the_condition_number(name):
    _, A, _, dmask, _, kappa = ref.structure_case(name)
    true = ref.kappa_scaled(A, dmask)
    print(f"{name}: cond(D^-1/2 A_FF D^-1/2) {true:.3f} <= {kappa:.3f}")
    assert 1.0 <= true <= kappa * (1 + 1e-12)


def test_symmetry_evidence_is_taken_on_summed_entries():
    mesh, _, _, dmask = ref.structure_case("hub321")[:4]
    r, c, a = ref.entries_of(mesh)
    amax = float(np.abs(a[~dmask[r] & ~dmask[c]]).max())
    assert ref.symmetry_evidence(r, c, a, dmask) == (0.0, amax, False)
    bad = ref.refused_matrices(r, c, a, dmask)
    (r1, c1, a1), _ = bad["v, v against v"]                 # 2 v against v
    k = len(r)
    assert ref.symmetry_evidence(r1, c1, a1, dmask)[0] == abs(a1[k]) > 1e-6 * amax
    assert ref.symmetry_evidence(*bad["no transposed entry"][0], dmask)[2] is True
    half = a1.copy()
    i = int(np.flatnonzero((r == r1[k]) & (c == c1[k]))[0])
    half[i] = half[k] = a[i] / 2                            # v / 2 + v / 2 against v
    assert ref.symmetry_evidence(r1, c1, half, dmask) == (0.0, amax, False)
    rp, cp, ap = ref.in_pieces(r, c, a, np.random.default_rng(9))
    S = ref.summed_entries(rp, cp, ap)
    assert len(S) == len(r) and len(rp) > 1.9 * len(r)
    assert max(abs(S[(i, j)] - v) for i, j, v in zip(r.tolist(), c.tolist(), a.tolist())) <= 2.0 ** -52 * amax
    defect, am, missing = ref.symmetry_evidence(rp, cp, ap, dmask)
    assert 0.0 < defect <= 1e-15 * amax and am == amax and not missing


def test_numpy_recurrences_stop_before_a_breakdown():
    A = ref.sp.csr_matrix(np.array([[1.0, 2.0], [2.0, 1.0]]))
    x, trace = ref.pcg_trace(A, np.array([1.0, 0.0]), np.zeros(2, bool), TOL, 10)
    assert x.tolist() == [1.0, 0.0] and trace == [1.0, 2.0]
    x0 = np.array([0.5, -0.25])
    x, trace = ref.pcg_trace(A, np.array([1.0, 0.0]), np.zeros(2, bool), TOL, 0, x0=x0)
    assert x.tolist() == x0.tolist() and trace == [1.25]   # max_iter 0: the start; r_0 = (1, 0) - A x_0 = (1, -0.75)
