"""GPU: the device Poisson reference solve (csrc/poisson_cg.hip) on the matrix structures its hexagon suite never builds -- row
lengths that differ inside a 64-row slice, slices of depth 0 or with one free lane, more than 256 block partials and more than 1 024
slices, every documented exit, every refusal of create, and positions given in pieces.

The matrices are tests/poisson_cg_ref.spd_problem's: strictly diagonally dominant (slack 0.25) with Dirichlet rows that are NOT
identity rows, so the truth is ``lifted_direct`` (spsolve on A_FF) and the error gate needs no eigensolver:
|x - u|_F / |u|_F <= kappa_gershgorin true_rel, kappa_gershgorin <= 9 bounding cond(D^-1/2 A_FF D^-1/2).  tests/test_host_poisson_cg.py
holds the numpy recurrences to the same gate on the same cases."""
import functools
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, pkg
import poisson_cg_ref as ref
from test_gpu_poisson_cg import ONE_FREE_NODE_FLOOR, rel_err_free

pytestmark = pytest.mark.gpu
TOL = 1e-12


def handle(dev, mesh, a_ij=None):
    eng = pkg("engine")
    b = mesh.to(dev)
    return eng.PoissonCG(eng.plan_for(b), b.a_ij if a_ij is None else a_ij), b


def check_case(what, out, y, dmask, u, kappa, tol=TOL):
    """What every case asserts: converged, true_rel <= 10 tol, the gate against u, Dirichlet rows bit-equal to y."""
    x = out["result"].cpu().numpy()[:, 0]
    err, lim = ref.gate(x, u, dmask, kappa, out["true_rel"])
    print(f"{what}: n_iter {out['n_iter']} true_rel {out['true_rel']:.3e} err {err:.3e} bound {lim:.3e} (kappa <= {kappa:.2f})")
    assert out["converged"] and out["true_rel"] <= 10 * tol
    assert err <= lim
    assert np.array_equal(x[dmask], y[dmask])
    return x


@pytest.mark.parametrize("name", ["hub321", "lonely", "band65536", "band65537"])
def test_structure_case_against_the_lifted_direct_solve(dev, name):
    mesh, A, y, dmask, u, kappa = ref.structure_case(name)
    cg, b = handle(dev, mesh)
    out = cg.solve(b.y, tol=TOL)
    cg.close()
    assert out["sym_defect"] == 0.0 and len(out["res_trace"]) == out["n_iter"] + 1
    x = check_case(name, out, y, dmask, u, kappa)
    if name == "lonely":
        # 1 x 1 blocks of A_FF: x_i = (y_i - sum_j a_ij y_j) / a_ii, to the floor of two correctly computed 1 x 1 solves
        rows = ref.one_by_one_rows(A, dmask)
        want = np.array([ref.one_by_one_solution(A, y, i) for i in rows])
        ulps = np.abs(x[rows] - want) / np.abs(want) / 2.0 ** -52
        print("1 x 1 rows", [int(i) for i in rows], "ulps", np.round(ulps, 2))
        assert {5, 10, 63, 127, 128} <= set(int(i) for i in rows)
        assert (np.abs(x[rows] - want) <= ONE_FREE_NODE_FLOOR * np.abs(want)).all()


def test_float32_hub_widens_exactly(dev):
    eng = pkg("engine")
    mesh, A, y, dmask, u, kappa = ref.structure_case("hub321_f32")
    b = mesh.to(dev)
    assert b.a_ij.dtype == torch.float32 and b.y.dtype == torch.float32
    plan = eng.plan_for(b)
    narrow = eng.PoissonCG(plan, b.a_ij).solve(b.y, tol=TOL)
    check_case("hub321 float32", narrow, y, dmask, u, kappa)     # the float64 solve of the same rounded values
    wide = eng.PoissonCG(plan, b.a_ij.double()).solve(b.y.double(), tol=TOL)
    assert torch.equal(narrow["result"], wide["result"])
    assert narrow["res_trace"] == wide["res_trace"] and narrow["n_iter"] == wide["n_iter"]


@functools.lru_cache(maxsize=None)
def hex148():
    """(mesh on the host, A, y, dirichlet mask) of the 66 157-node hexagon -- computed once, shared, never modified."""
    mesh = pkg("data").make_hex_problem(148, seed=148, compute_sol=False, dtype=torch.float64)
    return (mesh,) + ref.system(mesh)


def test_hexagon_past_65536_rows(dev):
    """The real matrix at 259 block partials and 1 034 slices (66 157 nodes); kappa needs an eigensolver here, so the gate is the
    reference recurrences' own error, 16 x (the convention of tests/recurrences.py): err_device <= 16 err_numpy, both against the
    direct solve.  Measured on the MI355X: n_iter 839 (numpy 839), true_rel 1.065e-12, err 3.561e-13 against numpy's 3.561e-13,
    so the 16 x gate stands at 5.698e-12."""
    eng = pkg("engine")
    mesh, A, y, dmask = hex148()
    assert mesh.num_nodes == 66157 and -(-mesh.num_nodes // 256) == 259
    u = ref.direct(A, y)
    x_np, want = ref.pcg_trace(A, y, dmask, TOL, eng.default_cg_max_iter(mesh.num_nodes))
    out = eng.poisson_solve(mesh.to(dev), tol=TOL)
    x = out["result"].cpu().numpy()[:, 0]
    err, err_np = rel_err_free(x, u, dmask), rel_err_free(x_np, u, dmask)
    print(f"hex148: n_iter {out['n_iter']} (numpy {len(want) - 1}) true_rel {out['true_rel']:.3e} err {err:.3e} "
          f"numpy's err {err_np:.3e} bound {16 * err_np:.3e}")
    assert out["converged"] and out["true_rel"] <= 10 * TOL
    assert err <= 16 * err_np
    assert np.array_equal(x[dmask], y[dmask])
    got = np.array(out["res_trace"][:10])
    assert len(got) == 10 and np.allclose(got, want[:10], rtol=1e-8, atol=0)


@pytest.mark.parametrize("name", ["hub321", "lonely", "band65537"])
def test_first_products_match_numpy(dev, name):
    """No convergence involved: from a random start, |r_0| / |b| (one product with the ELL) and, after max_iter = 1, |r_1| / |b|
    (a second one, through the direction kernel) equal numpy's to rtol = 4 N 2^-52 -- slack for the order of summation only (a row
    sum of up to 321 terms and a norm over N rows, each in a different order on the device).  A dropped, doubled or misplaced ELL
    entry changes these by far more."""
    mesh, A, y, dmask = ref.structure_case(name)[:4]
    N = mesh.num_nodes
    x0 = np.random.default_rng(N).standard_normal(N)
    _, want = ref.pcg_trace(A, y, dmask, TOL, 1, x0=x0)
    cg, b = handle(dev, mesh)
    out = cg.solve(b.y, x0=torch.from_numpy(x0)[:, None].to(dev), tol=TOL, max_iter=1)
    cg.close()
    got = out["res_trace"]
    rtol = 4 * N * 2.0 ** -52
    print(f"{name}: |r0|/|b| {got[0]:.17g} (numpy {want[0]:.17g}), |r1|/|b| {got[1]:.17g} (numpy {want[1]:.17g}), "
          f"rel diff {abs(got[0] / want[0] - 1):.2e} {abs(got[1] / want[1] - 1):.2e}, rtol {rtol:.2e}")
    assert out["n_iter"] == 1 and len(got) == 2 and len(want) == 2
    assert np.allclose(got, want, rtol=rtol, atol=0)


def test_two_handles_same_bits(dev):
    mesh = ref.structure_case("hub321")[0]
    outs = []
    for _ in range(2):
        cg, b = handle(dev, mesh.clone())
        outs.append(cg.solve(b.y, tol=TOL))
        cg.close()
    assert torch.equal(outs[0]["result"], outs[1]["result"])
    assert outs[0]["res_trace"] == outs[1]["res_trace"] and outs[0]["n_iter"] == outs[1]["n_iter"]
    assert (outs[0]["rel"], outs[0]["true_rel"]) == (outs[1]["rel"], outs[1]["true_rel"])


# ------------------------------------------------------------------------------------------------ every exit
BLOCK = ([0, 0, 1, 1], [0, 1, 1, 0], [1.0, 2.0, 1.0, 2.0])   # A = [[1, 2], [2, 1]]: eigenvalues 3 and -1


def test_breakdown_returns_the_iterate_before_it(dev):
    """y = (1, 0): p.Ap is 1 in the first iteration (alpha 1, x = (1, 0), r = (0, -2), beta 4) and (4, -2).(0, 6) = -12 in the second."""
    rng = np.random.default_rng(2)
    r, c, a = (np.array(v) for v in BLOCK)
    mesh = ref.mesh_of_entries(2, r, c, a, [1.0, 0.0], np.zeros(2, bool), rng)
    cg, b = handle(dev, mesh)
    out = cg.solve(b.y, tol=TOL)
    cg.close()
    assert out["converged"] is False and out["n_iter"] == 1
    assert out["result"].cpu().numpy()[:, 0].tolist() == [1.0, 0.0]
    assert len(out["res_trace"]) == 2 and np.isfinite(out["res_trace"]).all() and out["res_trace"] == [1.0, 2.0]


def test_breakdown_inside_a_larger_system(dev):
    """The same block and right-hand side as an extra component of hub321's graph: its negative p.Ap outweighs the rest's in the third
    iteration (numpy: p.Ap = 69, 9.0, then -13)."""
    rng = np.random.default_rng(3)
    mesh0, _, y0, dm0 = ref.structure_case("hub321")[:4]
    r0, c0, a0 = ref.entries_of(mesh0)
    N = 323
    r, c, a = np.append(r0, np.array(BLOCK[0]) + 321), np.append(c0, np.array(BLOCK[1]) + 321), np.append(a0, BLOCK[2])
    y, dmask = np.append(y0, [1.0, 0.0]), np.append(dm0, [False, False])
    mesh = ref.mesh_of_entries(N, r, c, a, y, dmask, rng)
    A = ref.system(mesh)[0]
    x_np, want = ref.pcg_trace(A, y, dmask, TOL, 1000)
    assert want[-1] > TOL and len(want) - 1 < 1000          # numpy stopped at p.q <= 0
    cg, b = handle(dev, mesh)
    out = cg.solve(b.y, tol=TOL, max_iter=1000)
    cg.close()
    x = out["result"].cpu().numpy()[:, 0]
    diff = float(np.linalg.norm(x - x_np) / np.linalg.norm(x_np))
    print(f"breakdown after {out['n_iter']} iterations (numpy {len(want) - 1}); iterate before it: rel diff to numpy {diff:.3e}")
    assert out["converged"] is False and out["n_iter"] == len(want) - 1
    assert np.isfinite(x).all() and np.isfinite(out["res_trace"]).all()
    assert diff <= 1e-12
    assert np.array_equal(x[dmask], y[dmask])


def test_zero_right_hand_side_with_a_start(dev):
    mesh, _, _, dmask = ref.structure_case("hub321")[:4]
    cg, b = handle(dev, mesh)
    x0 = torch.from_numpy(np.random.default_rng(4).standard_normal((321, 1))).to(dev)
    out = cg.solve(torch.zeros_like(b.y), x0=x0, tol=TOL)
    cg.close()
    x = out["result"].cpu().numpy()[:, 0]
    assert (x == 0.0).all() and not np.signbit(x[~dmask]).any()
    assert out["n_iter"] == 0 and out["converged"] and out["res_trace"] == [0.0] and out["true_rel"] == 0.0


def test_no_iterations_allowed(dev):
    mesh, _, y, dmask = ref.structure_case("hub321")[:4]
    cg, b = handle(dev, mesh)
    x0 = np.random.default_rng(5).standard_normal(321)
    out = cg.solve(b.y, x0=torch.from_numpy(x0)[:, None].to(dev), tol=TOL, max_iter=0)
    cg.close()
    x = out["result"].cpu().numpy()[:, 0]
    assert out["n_iter"] == 0 and out["converged"] is False and len(out["res_trace"]) == 1 and np.isfinite(out["res_trace"][0])
    assert np.array_equal(x[~dmask], x0[~dmask]) and np.array_equal(x[dmask], y[dmask])


def test_one_handle_several_right_hand_sides(dev):
    """Each solve on a used handle is bit-equal to the same solve on a fresh one; max_iter 3, then 7, then the default, so the trace
    buffer is reallocated twice."""
    mesh = ref.structure_case("hub321")[0]
    rng = np.random.default_rng(6)
    used, b = handle(dev, mesh)
    for k, max_iter in enumerate((3, 7, None, 5)):
        y = torch.from_numpy(rng.standard_normal((321, 1))).to(dev)
        got = used.solve(y, tol=TOL, max_iter=max_iter)
        fresh, _ = handle(dev, mesh)
        want = fresh.solve(y, tol=TOL, max_iter=max_iter)
        fresh.close()
        assert torch.equal(got["result"], want["result"]), k
        assert got["res_trace"] == want["res_trace"] and got["n_iter"] == want["n_iter"] == (max_iter or got["n_iter"])
        assert got["converged"] is (max_iter is None)
    used.close()


# ------------------------------------------------------------------------------------------------ create
def test_every_refusal_of_create(dev):
    """Each is a plain error return of create (nothing is solved with a refused matrix); the device is fine afterwards."""
    eng, nat = pkg("engine"), pkg("_native")
    mesh, _, y, dmask, u, kappa = ref.structure_case("hub321")
    rng = np.random.default_rng(7)
    r, c, a = ref.entries_of(mesh)
    for what, ((rr, cc, aa), msg) in ref.refused_matrices(r, c, a, dmask).items():
        b = ref.mesh_of_entries(321, rr, cc, aa, y, dmask, rng).to(dev)
        with pytest.raises(nat.NativeError, match=msg):
            eng.PoissonCG(eng.plan_for(b), b.a_ij)
        print("refused:", what)
    cg, b = handle(dev, mesh)
    check_case("after the refusals", cg.solve(b.y, tol=TOL), y, dmask, u, kappa)
    cg.close()


def test_a_defect_past_the_256th_block_is_found(dev):
    """The symmetry evidence is reduced like every sum here: a partial per 256-row block, then one block over the partials, 256 at
    a stride.  A skewed entry between two free rows past row 65 536 is seen by blocks 256.. only -- the second stride."""
    eng, nat = pkg("engine"), pkg("_native")
    mesh, _, _, dmask = hex148()
    r, c = mesh.edge_index
    free = torch.from_numpy(~dmask)
    far = torch.nonzero(free[r] & free[c] & (r != c) & (r >= 65536) & (c >= 65536))
    assert far.numel() > 100
    b = mesh.to(dev)
    skew = b.a_ij.clone()
    skew[int(far[50])] *= 1.01
    with pytest.raises(nat.NativeError, match="symmetric"):
        eng.PoissonCG(eng.plan_for(b), skew)
    cg = eng.PoissonCG(eng.plan_for(b), b.a_ij)         # the plain matrix is accepted with defect 0
    assert cg.solve(b.y, tol=TOL, max_iter=0)["sym_defect"] == 0.0
    cg.close()


def test_dirichlet_rows_are_never_read(dev):
    mesh, _, y, dmask = ref.structure_case("hub321")[:4]
    rng = np.random.default_rng(8)
    r, c, a = ref.entries_of(mesh)
    gr, gc, ga = ref.garbage_in_dirichlet_rows(r, c, a, dmask, rng)
    assert not np.isfinite(ga[dmask[gr]]).all() and not (dmask[gr] & (gr == gc)).any() and len(gr) < len(r)
    clean, b = handle(dev, mesh)
    dirty, bd = handle(dev, ref.mesh_of_entries(321, gr, gc, ga, y, dmask, rng))
    want, got = clean.solve(b.y, tol=TOL), dirty.solve(bd.y, tol=TOL)
    clean.close(), dirty.close()
    assert got["sym_defect"] == 0.0 and got["converged"]
    assert torch.equal(got["result"], want["result"]) and got["res_trace"] == want["res_trace"]
    assert (got["rel"], got["true_rel"]) == (want["rel"], want["true_rel"])


def test_matrix_given_in_pieces(dev):
    """A is the sum of the entries given for a position: the pieces of ref.in_pieces (v/2 + v/2 against v among them) are accepted,
    sym_defect is the numpy statement on the summed positions (the last bit of a sum of three pieces), and the solve meets the gate
    against the summed matrix."""
    mesh, _, y, dmask = ref.structure_case("hub321")[:4]
    rng = np.random.default_rng(9)
    r, c, a = ref.in_pieces(*ref.entries_of(mesh), rng)
    pieces = ref.mesh_of_entries(321, r, c, a, y, dmask, rng)
    A = ref.system(pieces)[0]                                   # scipy sums the pieces of a position
    defect, amax, missing = ref.symmetry_evidence(r, c, a, dmask)
    assert len(r) > 1.9 * mesh.num_edges and not missing and 0.0 < defect <= 1e-15 * amax
    cg, b = handle(dev, pieces)
    out = cg.solve(b.y, tol=TOL)
    cg.close()
    print(f"sym_defect {out['sym_defect']:.3e} (numpy on summed positions {defect:.3e})")
    assert out["sym_defect"] == defect
    check_case("hub321 in pieces", out, y, dmask, ref.lifted_direct(A, y, dmask), ref.kappa_gershgorin(A, dmask))


@pytest.mark.parametrize("mixed", [False, True])
def test_without_repeated_positions_nothing_changed(dev, mixed):
    """hex13: result, trace and sym_defect bit-equal to the build before create summed repeated positions
    (tests/golden/poisson_cg_hex13_parent.npz, recorded on the MI355X from that build)."""
    eng, data = pkg("engine"), pkg("data")
    rec = np.load(os.path.join(GOLDEN, "poisson_cg_hex13_parent.npz"))
    k = "mixed" if mixed else "dirichlet"
    out = eng.poisson_solve(data.make_hex_problem(13, seed=13, mixed=mixed, dtype=torch.float64).to(dev), tol=TOL)
    assert np.array_equal(out["result"].cpu().numpy()[:, 0], rec[k + "_result"])
    assert np.array_equal(np.array(out["res_trace"]), rec[k + "_trace"])
    assert out["sym_defect"] == float(rec[k + "_sym_defect"]) == 0.0
