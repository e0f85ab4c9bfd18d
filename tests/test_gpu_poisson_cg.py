"""GPU: the device Poisson reference solve (csrc/poisson_cg.hip: Jacobi-PCG in float64 on the plan's matrix structure) against the
host's direct solve.

Sizes: hexagons n = 1, 2, 13 (7, 19, 547 nodes: one free node, a partial wave, 8 full waves plus a 35-lane tail) in both families
and n = 58 (10 267 nodes: 41 blocks in every reduction).  The kernels have ONE reduction shape at every size (a partial per 256-row
block, then one block over the partials), so there is no switch-over size to straddle.

The error bound is derived, not guessed: for A_FF x = b, |x - u| / |u| <= kappa |b - A_FF x| / |b|, with kappa =
cond(D^-1/2 A_FF D^-1/2) computed here (numpy up to 547 nodes, scipy's eigsh at 10 267) and the solver's own ``true_rel``; it is
asserted as it stands on every mesh with more than one free node (there kappa true_rel is 1e-15 ... 1e-9).  The 7-node mesh has ONE
free node and kappa 1: the whole comparison sits at the float64 floor, where spsolve's u is itself only correct to an ulp or two
(measured there: true_rel 8.4e-17, |x - u| / |u| 1.9e-16 = one ulp).  That case alone is given ONE_FREE_NODE_FLOOR = 4 ulp of float64
on top of the bound: up to two roundings in each of the two 1 x 1 solves that are compared."""
import functools

import numpy as np
import pytest
import torch

from conftest import pkg
import poisson_cg_ref as ref

pytestmark = pytest.mark.gpu
TOL = 1e-12


@functools.lru_cache(maxsize=None)
def case(n, mixed, dtype=torch.float64):
    """(mesh on the host, A, y, dirichlet mask, direct solution, kappa) -- computed once, shared, never modified."""
    mesh = pkg("data").make_hex_problem(n, seed=n, mixed=mixed, dtype=dtype)
    A, y, dmask = ref.system(mesh, np.float32 if dtype == torch.float32 else np.float64)
    return mesh, A, y, dmask, ref.direct(A, y), ref.kappa_scaled(A, dmask)


ONE_FREE_NODE_FLOOR = 4 * 2.0 ** -52   # float64 ulps allowed between two correctly computed 1 x 1 solves (module docstring)


def bound(kappa, true_rel, n_free):
    return kappa * true_rel + (ONE_FREE_NODE_FLOOR if n_free == 1 else 0.0)


def rel_err_free(x, u, dmask):
    F = ~dmask
    return float(np.linalg.norm((x - u)[F]) / np.linalg.norm(u[F]))


def check_against_direct(out, n, mixed, dtype=torch.float64, tol=TOL):
    _, _, _, dmask, u, kappa = case(n, mixed, dtype)
    x = out["result"].cpu().numpy()[:, 0]
    err, lim = rel_err_free(x, u, dmask), bound(kappa, out["true_rel"], int((~dmask).sum()))
    print(f"n={n} mixed={mixed} {dtype}: n_iter {out['n_iter']} rel {out['rel']:.3e} true_rel {out['true_rel']:.3e} "
          f"kappa {kappa:.1f} err {err:.3e} bound {lim:.3e}")
    assert out["converged"] and out["true_rel"] <= 10 * tol
    assert err <= lim
    return x


@pytest.mark.parametrize("n,mixed", [(1, False), (1, True), (2, False), (2, True), (13, False), (13, True), (58, False), (58, True)])
def test_against_the_direct_solve(dev, n, mixed):
    eng = pkg("engine")
    out = eng.poisson_solve(case(n, mixed)[0].to(dev), tol=TOL)
    assert out["result"].shape == (3 * n * n + 3 * n + 1, 1) and out["result"].dtype == torch.float64
    assert len(out["res_trace"]) == out["n_iter"] + 1 and out["res_trace"][-1] == out["rel"]
    check_against_direct(out, n, mixed)


@pytest.mark.parametrize("mixed", [False, True])
def test_float32_inputs_widen_exactly(dev, mixed):
    eng = pkg("engine")
    b = case(13, mixed, torch.float32)[0].to(dev)
    assert b.a_ij.dtype == torch.float32 and b.y.dtype == torch.float32
    plan = eng.plan_for(b)
    narrow = eng.PoissonCG(plan, b.a_ij).solve(b.y, tol=TOL)
    check_against_direct(narrow, 13, mixed, torch.float32)      # the float64 direct solve of the same rounded values
    wide = eng.PoissonCG(plan, b.a_ij.double()).solve(b.y.double(), tol=TOL)
    assert torch.equal(narrow["result"], wide["result"])
    assert narrow["res_trace"] == wide["res_trace"] and narrow["n_iter"] == wide["n_iter"]


@pytest.mark.parametrize("mixed", [False, True])
def test_dirichlet_rows_hold_y_bitwise(dev, mixed):
    eng = pkg("engine")
    mesh, _, _, dmask = case(13, mixed)[:4]
    out = eng.poisson_solve(mesh.to(dev), tol=TOL)
    rows = torch.from_numpy(np.flatnonzero(dmask))
    assert rows.numel() == (78 if not mixed else 42)
    assert torch.equal(out["result"].cpu()[rows], mesh.y[rows])


def test_union_batch_is_one_block_diagonal_system(dev):
    eng, data = pkg("engine"), pkg("data")
    ns = (5, 13, 9)
    meshes = [case(n, False)[0] for n in ns]
    out = eng.poisson_solve(data.collate(meshes).to(dev), tol=TOL)
    assert out["converged"] and out["true_rel"] <= 10 * TOL
    x = out["result"].cpu().numpy()[:, 0]
    off, lam = 0, []
    for n, m in zip(ns, meshes):
        _, A, y, dmask, u, kappa = case(n, False)
        xb = x[off:off + m.num_nodes]
        off += m.num_nodes
        Aff, b, F = ref.lifted(A, y, dmask)
        true_rel = float(np.linalg.norm(b - Aff @ xb[F]) / np.linalg.norm(b))   # the block's own residual (the solver reports the union's)
        err = rel_err_free(xb, u, dmask)
        print(f"block n={n}: true_rel {true_rel:.3e} kappa {kappa:.1f} err {err:.3e} bound {kappa * true_rel:.3e}")
        assert err <= kappa * true_rel
        assert np.array_equal(xb[dmask], y[dmask])


def test_same_bits_whatever_the_polling(dev):
    eng = pkg("engine")
    b = case(13, True)[0].to(dev)
    cg = eng.PoissonCG(eng.plan_for(b), b.a_ij)
    a1, a2 = cg.solve(b.y, tol=TOL), cg.solve(b.y, tol=TOL)
    p1, p50 = cg.solve(b.y, tol=TOL, poll_every=1), cg.solve(b.y, tol=TOL, poll_every=50)
    for other in (a2, p1, p50):
        assert torch.equal(a1["result"], other["result"])
        assert a1["n_iter"] == other["n_iter"] and a1["res_trace"] == other["res_trace"]
        assert (a1["rel"], a1["true_rel"]) == (other["rel"], other["true_rel"])
    cg.close()


def test_budget(dev):
    eng = pkg("engine")
    out = eng.poisson_solve(case(13, False)[0].to(dev), tol=TOL, max_iter=5)
    assert out["converged"] is False and out["n_iter"] == 5
    assert len(out["res_trace"]) == 6 and np.isfinite(out["res_trace"]).all()
    assert bool(torch.isfinite(out["result"]).all())


def test_warm_start_from_the_solution(dev):
    eng = pkg("engine")
    mesh, _, _, dmask, u = case(13, False)[:5]
    out = eng.poisson_solve(mesh.to(dev), tol=1e-8, x0=torch.from_numpy(u)[:, None].to(dev))
    assert out["n_iter"] == 0 and out["converged"] and len(out["res_trace"]) == 1
    assert np.array_equal(out["result"].cpu().numpy()[~dmask, 0], u[~dmask])   # the start itself is returned


@pytest.mark.parametrize("mixed", [False, True])
def test_early_trace_matches_the_numpy_recurrences(dev, mixed):
    eng = pkg("engine")
    mesh, A, y, dmask = case(13, mixed)[:4]
    out = eng.poisson_solve(mesh.to(dev), tol=TOL)
    _, want = ref.pcg_trace(A, y, dmask, TOL, 20)
    got = np.array(out["res_trace"][:10])
    print("trace", got, "max rel diff", np.abs(got / np.array(want[:10]) - 1).max())
    assert len(got) == 10 and np.allclose(got, want[:10], rtol=1e-8, atol=0)


def test_refuses_a_matrix_cg_cannot_solve(dev):
    eng, nat = pkg("engine"), pkg("_native")
    mesh, _, _, dmask = case(13, False)[:4]
    b = mesh.to(dev)
    plan = eng.plan_for(b)
    r, c = mesh.edge_index
    free = torch.from_numpy(~dmask)
    off = int(torch.nonzero(free[r] & free[c] & (r != c))[7])
    skew = b.a_ij.clone()
    skew[off] *= 1.01
    with pytest.raises(nat.NativeError, match="symmetric"):
        eng.PoissonCG(plan, skew)
    dg = int(torch.nonzero(free[r] & (r == c))[3])
    nodiag = b.a_ij.clone()
    nodiag[dg] = 0.0
    with pytest.raises(nat.NativeError, match="diagonal"):
        eng.PoissonCG(plan, nodiag)
    assert eng.PoissonCG(plan, b.a_ij).solve(b.y, tol=TOL)["converged"]   # plain error returns: the device is fine afterwards


@pytest.mark.parametrize("mixed", [False, True])
def test_generator_device_solution(dev, mixed):
    data = pkg("data")
    host = data.make_hex_problem(13, seed=2, mixed=mixed, compute_sol=True)
    with torch.cuda.device(dev):
        devm = data.make_hex_problem(13, seed=2, mixed=mixed, compute_sol="device")
    assert devm.sol.dtype == torch.float32 and devm.sol.device.type == "cpu"
    a, b = host.sol.numpy(), devm.sol.numpy()
    ulp = np.spacing(np.maximum(np.abs(a), np.abs(b)))
    print("entries that differ", int((a != b).sum()), "max |diff| / ulp", float((np.abs(a - b) / ulp).max()))
    assert (np.abs(a - b) <= ulp).all()
    assert sorted(host.keys()) == sorted(devm.keys())
    for k in host.keys():
        if k != "sol":
            assert torch.equal(getattr(host, k), getattr(devm, k)), k
