"""GPU: the opt-in restarted GMRES for the implicit backward's adjoint system (csrc/krylov.hip ``adjoint_gmres_loop``,
``engine.DeviceGmres.solve_adjoint``, model config key ``bw_solver = "gmres"``).

Truth per case: float64 GMRES to 1e-13 on the float64 oracle VJP (tests/adjoint_gmres_ref.py), on the CPU.  H* is the oracle's fp32
Broyden fixed point at 1e-6, grad a seeded Gaussian; both routes on the GPU get exactly these tensors.

Gates (set by the issue).  Error of ``result`` against the truth <= 2 x the error of the existing Broyden adjoint route
(``DeviceBroyden.solve_adjoint``, same ``lin``, same inputs, 1e-8 / 500) measured in the same test, and products <= that route's.
Why 2: both routes end at the fp32 floor, where the CPU probe's ratio scatters between 0.4 and 1.2 over the fixtures; a wrong
sign, a missing restart or a broken gate is off by orders of magnitude.  ``lowest`` against the test's own recomputation from the
same operator and the returned vector: 1e-4 relative (the same fp32 vectors summed in another order).  Training-step gradients:
the criterion of tests/test_gpu_training.py::test_training_step_gradients, unchanged."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import adjoint_gmres_ref as ref
from conftest import CASES, load_case, load_weights, pkg
from test_gpu_training import _fp64_training_step, _model, _worst

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
M = 50
EPS, BUDGET = 1e-8, 500    # the launch configuration of the reference's backward (bw_tol, bw_thres)

# (fixture, n_layers, tile_target, lin: None = direct VJP, else the Linearization's ``neumann``)
LIN_CASES = [("hex13_dirichlet_s0", 1, 0, "direct"), ("hex26_dirichlet_s0", 1, 0, "direct"), ("hex13_mixed_s1", 1, 0, "direct"),
             ("hex13_mixed_s1", 1, 0, "stored")]
DIRECT_CASES = [("hex13_dirichlet_s0", 2, 0, None), ("hex13_dirichlet_s0", 1, -1, None)]


@functools.lru_cache(maxsize=None)
def _problem(name, L):
    return ref.AdjointProblem(name, sd=ref.stacked_dirichlet(L) if L > 1 else None)


def _bind(name, L, tt, lin, dev):
    """(problem, fmap, H*, grad, Linearization or None) on the device."""
    eng = pkg("engine")
    P = _problem(name, L)
    md = P.mesh.to(dev)
    plan = eng.plan_for(md) if tt == 0 else eng.MeshPlan(md, tile_target=tt)
    assert bool(plan.tiled) == (tt != -1)
    fmap = eng.FixedPointMap(plan, eng.PackedWeights(P.sd, dev), P.h0.to(dev), md.prb_data, getattr(md, "unit_normal_vector", None))
    H, g = P.h_star.to(dev), P.grad.to(dev)
    handle = None
    if lin is not None:
        assert fmap.can_linearize()
        handle = fmap.linearize_p(fmap.to_plan(H), neumann=lin)
        assert handle.neumann_stored == (lin == "stored" and bool(plan.mixed))
    return P, fmap, H, g, handle


def _gmres(fmap, dev, m=M):
    return pkg("engine").DeviceGmres(fmap.plan.N * 10, dev, m)


def _rel_of(fmap, H, g, lin, y):
    """|f(y) - y| / (|f(y)| + 1e-9), f(y) = J^T y + grad, from the operator the solve ran on; fp32 vectors, float64 sums."""
    if lin is not None:
        yp = fmap.to_plan(y)
        f = lin.vjp_p(yp) + fmap.to_plan(g)
    elif fmap.plan.tiled:
        yp = fmap.to_plan(y)
        f = fmap.vjp_p(fmap.to_plan(H), yp) + fmap.to_plan(g)
    else:
        yp = y
        f = fmap.vjp(H, y) + g
    r = f - yp
    return float(r.double().norm()) / (float(f.double().norm()) + 1e-9)


def _same(a, b):
    assert torch.equal(a["result"], b["result"])
    for k in ("nstep", "n_cycles", "stop", "lowest", "rel_trace", "abs_trace", "n_reorth"):
        assert a[k] == b[k], (k, a[k], b[k])


@pytest.mark.parametrize("name,L,tt,lin", LIN_CASES + DIRECT_CASES)
def test_error_and_products_against_the_broyden_route(name, L, tt, lin, dev):
    eng = pkg("engine")
    P, fmap, H, g, handle = _bind(name, L, tt, lin, dev)
    bro_sv = eng.DeviceBroyden(plan=fmap.plan, threshold=BUDGET, keep_trace=False)
    bro = bro_sv.solve_adjoint(fmap, H, g, EPS, lin=handle)
    gm_sv = _gmres(fmap, dev)
    out = gm_sv.solve_adjoint(fmap, H, g, EPS, BUDGET, lin=handle)
    e_gm, e_br = P.error(out["result"]), P.error(bro["result"])
    print(f"ADJOINT_GMRES {name} L={L} tt={tt} lin={lin}: GMRES({M}) products {out['nstep']} cycles {out['n_cycles']} stop {out['stop']} "
          f"lowest {out['lowest']:.3e} second passes {out['n_reorth']} error {e_gm:.3e} | Broyden products {bro['n_iter']} "
          f"lowest {bro['lowest']:.3e} error {e_br:.3e} | ratio {e_gm / e_br:.2f} | state bytes GMRES {gm_sv.nbytes} Broyden {bro_sv.nbytes}")
    assert bool(torch.isfinite(out["result"]).all())
    assert e_gm <= 2.0 * e_br, (e_gm, e_br)
    assert out["nstep"] <= bro["n_iter"], (out["nstep"], bro["n_iter"])
    # trace check: lowest belongs to the returned vector
    rel = _rel_of(fmap, H, g, handle, out["result"])
    assert abs(rel - out["lowest"]) <= 1e-4 * rel, (rel, out["lowest"])
    assert len(out["rel_trace"]) == len(out["abs_trace"]) == out["n_cycles"] and out["lowest"] == min(out["rel_trace"])
    assert out["rel_trace"][0] == pytest.approx(1.0, abs=1e-6)   # y_0 = 0: r = f(0) = grad
    for o in (bro_sv, gm_sv) + ((handle,) if handle is not None else ()):
        o.close()


# per case: does eps = 1e-4 end inside the first cycle (the CPU restatement needs 35 / 51 / 5 products there: the mixed fixture's first
# cycle runs all m steps), and a budget that ends the solve before it stagnates (the CPU restatement stagnates after 74 / 114 / 13)
@pytest.mark.parametrize("name,L,tt,lin,first_cycle,small_budget", [LIN_CASES[0] + (True, 30), LIN_CASES[3] + (False, 30),
                                                                    DIRECT_CASES[0] + (True, 6)])
def test_stops(name, L, tt, lin, first_cycle, small_budget, dev):
    P, fmap, H, g, handle = _bind(name, L, tt, lin, dev)
    sv = _gmres(fmap, dev)
    # tolerance: reached inside the first cycle, confirmed by the second cycle's residual
    out = sv.solve_adjoint(fmap, H, g, 1e-4, BUDGET, lin=handle)
    print(f"ADJOINT_GMRES stops {name} L={L}: eps 1e-4 -> {out['stop']} after {out['nstep']} products, {out['n_cycles']} cycles, lowest {out['lowest']:.3e}")
    assert out["stop"] == "tolerance" and out["lowest"] < 1e-4
    if first_cycle:
        assert out["nstep"] < M and out["n_cycles"] == 2, (out["nstep"], out["n_cycles"])
    rel = _rel_of(fmap, H, g, handle, out["result"])
    assert abs(rel - out["lowest"]) <= 1e-4 * rel
    # stagnation: 1e-8 is below fp32 resolution
    out = sv.solve_adjoint(fmap, H, g, EPS, BUDGET, lin=handle)
    print(f"ADJOINT_GMRES stops {name} L={L}: eps 1e-8 -> {out['stop']} after {out['nstep']} products, {out['n_cycles']} cycles, lowest {out['lowest']:.3e}")
    assert out["stop"] == "stagnation" and out["nstep"] < BUDGET
    # budget: the count never passes it, and the result is still the measured best
    out = sv.solve_adjoint(fmap, H, g, EPS, small_budget, lin=handle)
    assert out["stop"] == "budget" and out["nstep"] == small_budget and out["n_cycles"] == 2, (out["stop"], out["nstep"], out["n_cycles"])
    rel = _rel_of(fmap, H, g, handle, out["result"])
    assert abs(rel - out["lowest"]) <= 1e-4 * rel
    # zero right-hand side
    out = sv.solve_adjoint(fmap, H, torch.zeros_like(g), EPS, BUDGET, lin=handle)
    assert out["nstep"] == 0 and out["stop"] == "tolerance" and out["n_cycles"] == 1
    assert bool((out["result"] == 0).all()) and np.isfinite(out["lowest"]) and all(np.isfinite(out["rel_trace"]))
    # a solve after it is not disturbed by what the handle held
    again = sv.solve_adjoint(fmap, H, g, 1e-4, BUDGET, lin=handle)
    assert again["stop"] == "tolerance" and bool(torch.isfinite(again["result"]).all())
    sv.close()


@pytest.mark.parametrize("name,L,tt,lin", [LIN_CASES[1], LIN_CASES[3], DIRECT_CASES[0], DIRECT_CASES[1]])
def test_reproducible_and_independent_of_polling(name, L, tt, lin, dev):
    P, fmap, H, g, handle = _bind(name, L, tt, lin, dev)
    sv = _gmres(fmap, dev)
    for eps in (EPS, 1e-4):   # (1e-4: the cycle ends between two polls)
        base = sv.solve_adjoint(fmap, H, g, eps, BUDGET, lin=handle)
        _same(base, sv.solve_adjoint(fmap, H, g, eps, BUDGET, lin=handle))
        for poll in (1, 8, M):
            _same(base, sv.solve_adjoint(fmap, H, g, eps, BUDGET, lin=handle, poll_every=poll))
    other = _gmres(fmap, dev)   # another handle, another basis
    _same(base, other.solve_adjoint(fmap, H, g, 1e-4, BUDGET, lin=handle))
    sv.close()
    other.close()


def test_profile_names(dev):
    """The new kernels are accounted by psignn_prof_* under their own names, with the bytes stated at the launch sites."""
    nat = pkg("_native")
    P, fmap, H, g, handle = _bind(*LIN_CASES[0], dev)
    sv = _gmres(fmap, dev)
    nat.prof_enable(True)
    nat.prof_collect()
    out = sv.solve_adjoint(fmap, H, g, EPS, BUDGET, lin=handle)
    ran = nat.prof_collect(with_bytes=True)
    nat.prof_enable(False)
    vb = fmap.plan.N * 10 * 4
    assert ran["k_ag_begin"][0] == ran["k_ag_check"][0] == ran["k_ag_keep"][0] == out["n_cycles"]
    assert ran["k_ag_begin"][2] == 3 * vb + 4 * vb * (out["n_cycles"] - 1) and ran["k_ag_keep"][2] == 2 * vb * out["n_cycles"]
    assert ran["k_vjp_lin"][0] >= out["nstep"] and ran["k_gm_finish"][0] >= out["nstep"] - (out["n_cycles"] - 1)
    assert "k_xnext" not in ran and "k_addv" not in ran   # nothing of the Broyden loop ran
    sv.close()


def _draw(name, draw):
    _, mesh = load_case(name)
    m = mesh.clone()
    if draw > 0:
        gen = torch.Generator().manual_seed(2000 + draw)
        m.x = mesh.x * (1 + 1e-7 * torch.randn(mesh.x.shape, generator=gen))
    return m


@pytest.mark.parametrize("linearize", [False, True])
@pytest.mark.parametrize("name", ["hex13_dirichlet_s0", "original_dirichlet_s0", "hex13_mixed_s1"])
def test_training_step_gradients_with_gmres_backward(name, linearize, dev):
    """loss.backward() with ``bw_solver = "gmres"`` on the four stored inputs of grad_truth_fp64.npz; the criterion of
    test_training_step_gradients: every run within 1e-2, the mean of the worst-tensor errors within max(5e-3, 1.25 x the reference
    path's mean)."""
    sd = load_weights(CASES[name])
    band = json.load(open(os.path.join(GOLDEN, "grad_error_band.json")))[name]
    T = np.load(os.path.join(GOLDEN, "grad_truth_fp64.npz"))
    kw = dict(fw_tol=1e-7, fw_thres=600, bw_solver="gmres")
    if linearize:
        kw["bw_linearize"] = True
        if CASES[name] == "mixed":
            kw["lin_neumann"] = "stored"
    errs, steps = [], []
    for draw in range(4):
        net = _model(sd, dev, **kw).train()
        u, ld = net(_draw(name, draw).to(dev))
        (ld["residual_loss"] + ld["encoder_loss"] + ld["autoencoder_loss"]).backward()
        bw = net.deqdss.last_backward
        assert bw["stop"] in ("tolerance", "stagnation") and bw["lowest"] < 1e-6 and bw["threshold"] == 400, bw["stop"]
        steps.append(bw["nstep"])
        got = {k: p.grad for k, p in net.named_parameters()}
        assert all(v is not None for v in got.values())
        want = {k: torch.from_numpy(T[f"{name}/{draw}/{k}"]) for k in got}
        scale = max(float(t.norm()) for t in want.values())
        e, k = _worst(got, want, scale)
        errs.append(e)
        assert e < 1e-2, (draw, k, e)
    print(f"ADJOINT_GMRES training {name} linearize={linearize}: worst-tensor gradient errors vs fp64 truth "
          f"{['%.2e' % e for e in errs]}, mean {np.mean(errs):.2e}; reference path mean {band['mean']:.2e}; products {steps}")
    assert np.mean(errs) <= max(5e-3, 1.25 * band["mean"]), (errs, band["mean"])


@pytest.mark.parametrize("name", ["hex13_dirichlet_s0", "hex13_mixed_s1"])
def test_training_step_with_regulariser_and_gmres_backward(name, dev):
    """jac_weight = 1 (the reference's launch scripts): the Jacobian regulariser's gradient joins the hooked one.  One run against
    the float64 step with the same probe: the single-run bound 1e-2."""
    _, mesh = load_case(name)
    sd = load_weights(CASES[name])
    net = _model(sd, dev, fw_tol=1e-7, fw_thres=600, bw_solver="gmres").train()
    u, ld = net(mesh.to(dev))
    assert ld["jacobian_loss"].requires_grad
    (ld["residual_loss"] + 1.0 * ld["jacobian_loss"] + ld["encoder_loss"] + ld["autoencoder_loss"]).backward()
    assert net.deqdss.last_backward["stop"] in ("tolerance", "stagnation")
    got = {k: p.grad for k, p in net.named_parameters()}
    _, _, want, _, _ = _fp64_training_step(sd, mesh, jac_weight=1.0, probe=net.deqdss.last_probe.cpu())
    want = {k: want[k] for k in got}
    scale = max(float(t.norm()) for t in want.values())
    e, k = _worst(got, want, scale)
    print(f"ADJOINT_GMRES training {name} jac_weight=1: worst-tensor gradient error vs fp64 truth {e:.2e} ({k})")
    assert e < 1e-2, (k, e)


@pytest.mark.parametrize("name", ["hex13_dirichlet_s0", "hex13_mixed_s1"])
def test_default_route_unchanged(name, dev):
    """Key absent, or None: the same bits as a model that never heard of it, and the Broyden dict (no GMRES fields)."""
    _, mesh = load_case(name)
    sd = load_weights(CASES[name])
    grads = []
    for kw in ({}, {"bw_solver": None}, {"bw_gmres_m": 20}):
        net = _model(sd, dev, fw_tol=1e-7, fw_thres=600, **kw).train()
        u, ld = net(mesh.to(dev))
        (ld["residual_loss"] + ld["encoder_loss"] + ld["autoencoder_loss"]).backward()
        assert "n_cycles" not in net.deqdss.last_backward and "n_iter" in net.deqdss.last_backward
        grads.append({k: p.grad.clone() for k, p in net.named_parameters()})
    for other in grads[1:]:
        assert all(torch.equal(grads[0][k], other[k]) for k in grads[0])


@pytest.mark.parametrize("family", ["dirichlet", "mixed"])
def test_replicas_solve_one_after_the_other(family, dev):
    """DataParallel(replicas=2) with the key: no lockstep route, each replica's adjoint solve is the single-batch one -- the same
    bits in its solver dict -- and the parameter gradient of the summed loss is the sum of the single-batch gradients."""
    loader, nat = pkg("loader"), pkg("_native")
    names = [("hex13_dirichlet_s0", 0), ("original_dirichlet_s0", 0)] if family == "dirichlet" else [("hex13_mixed_s1", 0), ("hex13_mixed_s1", 1)]
    sd = load_weights(family)
    meshes = [_draw(n, d) for n, d in names]
    kw = dict(fw_tol=1e-7, fw_thres=600, bw_solver="gmres", bw_linearize=True)
    if family == "mixed":
        kw["lin_neumann"] = "stored"
    net = _model(sd, dev, **kw).train()
    wrapped = loader.DataParallel(net, replicas=2).to(dev)
    us, ld = wrapped(meshes)
    assert ld["residual_loss"].shape == (2,)
    nat.prof_enable(True)
    nat.prof_collect()
    (ld["residual_loss"] + ld["encoder_loss"] + ld["autoencoder_loss"]).sum().backward()
    ran = nat.prof_collect()
    nat.prof_enable(False)
    assert "k_vjp_lin_batch" not in ran and "k_ag_check" in ran and "k_xnext" not in ran, sorted(ran)
    bws = net.deqdss.last_backward
    assert len(bws) == 2 and all(o["stop"] in ("tolerance", "stagnation") for o in bws)
    got = {k: p.grad.clone() for k, p in net.named_parameters()}
    singles = []
    for r, m in enumerate(meshes):
        one = _model(sd, dev, **kw).train()
        u, l1 = one(m.to(dev))
        (l1["residual_loss"] + l1["encoder_loss"] + l1["autoencoder_loss"]).backward()
        _same(one.deqdss.last_backward, bws[r])
        singles.append({k: p.grad.clone() for k, p in one.named_parameters()})
    for k in got:
        want = singles[0][k].double() + singles[1][k].double()
        assert float((got[k].double() - want).norm()) <= 1e-5 * max(float(want.norm()), 1e-30), k
