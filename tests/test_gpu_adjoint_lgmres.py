"""GPU: augmented restarts (LGMRES) and the stall ratio of the fp32 GMRES adjoint solve (csrc/krylov.hip ``k_lg_check``,
``k_lg_shift``, ``k_lg_combine``, ``k_lg_norm``; ``engine.DeviceGmresAug``; model keys ``bw_gmres_augment`` / ``bw_gmres_stall``).

Problems: those of tests/test_gpu_adjoint_gmres.py (``_problem`` / ``_bind``: shipped checkpoint, H* from the oracle's fp32 Broyden,
a seeded Gaussian grad; 547 - 2 107 nodes).  The short restart m = 10 is the test ground: the default m = 50 hides the halving rule on
these fixtures.

Gates.  Counts against the restatement ``lgmres_ref.lgmres_adjoint`` driven by the device's own fp32 product (``lin.vjp_p``, which is
not the code under test): the same stop reason, ``n_cycles`` within 1, products within m + 1 (the stop tests act once per cycle, so a
rounding difference moves the end by at most a cycle).  ``lowest`` against the test's own recomputation from the returned vector:
1e-4 relative, the rule of ``_rel_of``.  ``result`` against the restatement's: ``RESULT_GATE`` = 250 x the restatement's own spread
under 4-ulp perturbations of every product (scripts/calib_adjoint_lgmres.py: 6.87e-6 over the ten runs that end on "tolerance", no
count moved), the factor the project uses elsewhere.  Accuracy at the launch tolerance (eps 1e-8, budget 500, m 10): error to
``AdjointProblem.truth()`` above 1e-2 with (0, 0.5) and below 1e-3 with (1, 1.0) -- the CPU restatement gives 1.2e-1 / 6.6e-2 and
1.0e-5 / 8.0e-6, four orders of magnitude apart.  Training-step gradients: every tensor within 1e-2 of grad_truth_fp64.npz, the
single-run bound of tests/test_gpu_adjoint_gmres.py::test_training_step_gradients_with_gmres_backward.

On the MI355X, one run: every count equal to the restatement's in all 11 compared runs, results 1.4e-7 - 2.4e-6 from it; errors at the
launch tolerance 1.16e-1 / 5.99e-2 with (0, 0.5) and 1.48e-6 / 1.06e-5 with (1, 1.0); products(1, 1.0) / products(0, 1.0) = 0.56 / 0.57
(hex13 mixed, hex26) and 0.62 (hex13 dirichlet)."""
import os

import numpy as np
import pytest
import torch

import handle_reuse as hr
import lgmres_ref as lg
from conftest import CASES, load_weights, pkg
from test_gpu_adjoint_gmres import _bind, _draw, _rel_of, _same
from test_gpu_training import _model, _worst

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
M, EPS, BUDGET = 10, 1e-5, 800
RESULT_GATE = 250 * 6.87e-6   # scripts/calib_adjoint_lgmres.py
WIDE = 1 << 20                # shard_elems past the 786 432-element switch: 16 floats per lane

# (fixture, n_layers, tile_target, lin) as in tests/test_gpu_adjoint_gmres.py
LIN = {"hex13_dirichlet_s0": ("hex13_dirichlet_s0", 1, 0, "direct"), "hex26_dirichlet_s0": ("hex26_dirichlet_s0", 1, 0, "direct"),
       "hex13_mixed_s1": ("hex13_mixed_s1", 1, 0, "stored")}
SAME_BITS_CASES = [LIN["hex13_dirichlet_s0"], LIN["hex13_mixed_s1"], ("hex13_mixed_s1", 1, 0, None), ("hex13_dirichlet_s0", 1, -1, None),
                   ("hex13_dirichlet_s0", 2, 0, None)]
_bound, _dev_runs, _ref_runs = {}, {}, {}


def _bound_case(case, dev):
    key = case + (str(dev),)
    if key not in _bound:
        _bound[key] = _bind(*case, dev)
    return _bound[key]


def _aug(fmap, dev, m=M, augment=2, shard_elems=None):
    return pkg("engine").DeviceGmresAug(fmap.plan.N * 10, dev, m, augment=augment, shard_elems=shard_elems)


def _dev_run(case, dev, augment, stall, eps=EPS, budget=BUDGET, shard_elems=None):
    """One device solve on a fresh handle of ``augment`` kept corrections, computed once and shared."""
    key = (case, str(dev), augment, stall, eps, budget, shard_elems)
    if key not in _dev_runs:
        P, fmap, H, g, handle = _bound_case(case, dev)
        sv = _aug(fmap, dev, augment=augment, shard_elems=shard_elems)
        _dev_runs[key] = sv.solve_adjoint(fmap, H, g, eps, budget, lin=handle, stall=stall)
        sv.close()
    return _dev_runs[key]


def _ref_run(case, dev, augment, stall, eps=EPS, budget=BUDGET):
    """The restatement on the device's own fp32 product (plan order), computed once and shared; ``result`` in the caller's numbering."""
    key = (case, str(dev), augment, stall, eps, budget)
    if key not in _ref_runs:
        P, fmap, H, g, handle = _bound_case(case, dev)
        out = lg.lgmres_adjoint(handle.vjp_p, fmap.to_plan(g), eps, budget, m=M, augment=augment, stall=stall, device=dev)
        out["result"] = fmap.from_plan(out["result"])
        _ref_runs[key] = out
    return _ref_runs[key]


def _against_restatement(label, case, dev, out, augment, stall, eps=EPS, budget=BUDGET):
    """Check 4 of the module docstring."""
    P, fmap, H, g, handle = _bound_case(case, dev)
    want = _ref_run(case, dev, augment, stall, eps, budget)
    dist = float((out["result"].double() - want["result"].double()).norm() / want["result"].double().norm())
    rel = _rel_of(fmap, H, g, handle, out["result"])
    print(f"ADJOINT_LGMRES {label} ({augment}, {stall}): device {out['nstep']} products, {out['n_cycles']} cycles, n_aug {out['n_aug']}, "
          f"{out['stop']}, lowest {out['lowest']:.3e} (recomputed {rel:.3e}) | restatement {want['nstep']} products, {want['n_cycles']} cycles, "
          f"n_aug {want['n_aug']}, {want['stop']}, lowest {want['lowest']:.3e} | result distance {dist:.2e} (gate {RESULT_GATE:.2e}) | "
          f"counts equal: {all(out[k] == want[k] for k in ('nstep', 'n_cycles', 'n_aug', 'n_reorth'))}")
    assert out["stop"] == want["stop"], (label, out["stop"], want["stop"])
    assert abs(out["n_cycles"] - want["n_cycles"]) <= 1, (label, out["n_cycles"], want["n_cycles"])
    assert abs(out["nstep"] - want["nstep"]) <= M + 1, (label, out["nstep"], want["nstep"])
    assert abs(rel - out["lowest"]) <= 1e-4 * rel, (label, rel, out["lowest"])
    assert len(out["rel_trace"]) == len(out["abs_trace"]) == out["n_cycles"] and out["lowest"] == min(out["rel_trace"])
    assert bool(torch.isfinite(out["result"]).all())
    assert dist <= RESULT_GATE, (label, dist)


# ------------------------------------------------------------------------------------------------------------- 1. same bits at defaults
@pytest.mark.parametrize("m", [50, 10])
@pytest.mark.parametrize("case", SAME_BITS_CASES, ids=lambda c: f"{c[0]}-L{c[1]}-tt{c[2]}-{c[3]}")
def test_defaults_give_the_bits_and_launches_of_device_gmres(case, m, dev):
    eng, nat = pkg("engine"), pkg("_native")
    P, fmap, H, g, handle = _bound_case(case, dev)
    plain_sv = eng.DeviceGmres(fmap.plan.N * 10, dev, m)
    nb_plain = plain_sv.nbytes   # (before the first solve makes the workspace)
    # the first transposed product on a linearisation builds its reverse tables once (k_lin_rev, k_lin_tfill): that belongs to the
    # handle `lin`, not to a solve, so it is done before the launches of the three solves are compared
    plain_sv.solve_adjoint(fmap, H, g, 1e-8, 2, lin=handle)
    nat.prof_enable(True)
    nat.prof_collect()
    want = plain_sv.solve_adjoint(fmap, H, g, 1e-8, 500, lin=handle)
    ran_plain = nat.prof_collect()
    outs = []
    for augment, kw in ((2, dict(augment=0, stall=0.5)), (0, {})):
        sv = _aug(fmap, dev, m=m, augment=augment)
        assert sv.nbytes - nb_plain == ((augment + 1) * sv.ld * 4 if augment else 0)
        outs.append(sv.solve_adjoint(fmap, H, g, 1e-8, 500, lin=handle, **kw))
        ran = nat.prof_collect()
        assert not any(k.startswith("k_lg_") for k in ran), sorted(ran)
        assert {k: v[0] for k, v in ran.items()} == {k: v[0] for k, v in ran_plain.items()}   # the same launches, kernel by kernel
        sv.close()
    nat.prof_enable(False)
    for out in outs:
        _same(out, want)
        assert out["n_aug"] == 0 and out["augment"] == 0 and out["lowest_abs"] == want["lowest_abs"]
    assert want["n_cycles"] >= 2
    plain_sv.close()


# ------------------------------------------------------------------------------------------------------------- 2. both vector widths
def test_both_vector_widths(dev):
    case = LIN["hex13_mixed_s1"]
    P, fmap, H, g, handle = _bound_case(case, dev)
    outs = {}
    for shard in (WIDE, None):
        sv = _aug(fmap, dev, augment=2, shard_elems=shard)
        base = sv.solve_adjoint(fmap, H, g, EPS, BUDGET, lin=handle, stall=1.0)
        for poll in (1, 8, 1000):   # within a width: the same bits whatever the polling
            again = sv.solve_adjoint(fmap, H, g, EPS, BUDGET, lin=handle, stall=1.0, poll_every=poll)
            hr.same_out(again, base, ("width", shard, "poll_every", poll))
        sv.close()
        _against_restatement(f"hex13_mixed_s1 stored, shard_elems {shard}", case, dev, base, 2, 1.0)
        outs[shard] = base
    assert outs[WIDE]["stop"] == outs[None]["stop"] and outs[WIDE]["n_cycles"] == outs[None]["n_cycles"]


# ------------------------------------------------------------------------------------------------------------- 3. + 4.
@pytest.mark.parametrize("name", ["hex13_mixed_s1", "hex26_dirichlet_s0"])
def test_the_rule_and_the_corrections(name, dev):
    case = LIN[name]
    plain, lifted, one = (_dev_run(case, dev, a, s) for a, s in ((0, 0.5), (0, 1.0), (1, 1.0)))
    print(f"ADJOINT_LGMRES {name}: (0, 0.5) {plain['nstep']} {plain['stop']} lowest {plain['lowest']:.2e} | (0, 1.0) {lifted['nstep']} "
          f"{lifted['stop']} | (1, 1.0) {one['nstep']} {one['stop']} n_aug {one['n_aug']} | ratio {one['nstep'] / lifted['nstep']:.2f}")
    assert plain["stop"] == "stagnation" and plain["lowest"] > 1e-4
    assert lifted["stop"] == "tolerance" and one["stop"] == "tolerance"
    assert one["nstep"] <= 0.75 * lifted["nstep"], (one["nstep"], lifted["nstep"])
    for augment, out in ((0, plain), (0, lifted), (1, one)):
        assert out["n_cycles"] >= 3 and out["augment"] == augment
        assert (out["n_aug"] > 0) == (augment > 0) and out["n_aug"] <= augment * (out["n_cycles"] - 1)
    for (augment, stall), out in (((0, 0.5), plain), ((0, 1.0), lifted), ((1, 1.0), one)):
        _against_restatement(name, case, dev, out, augment, stall)


def test_kept_corrections_cut_the_products_where_the_rule_does_not_bite(dev):
    case = LIN["hex13_dirichlet_s0"]
    lifted, one, two = (_dev_run(case, dev, a, 1.0) for a in (0, 1, 2))
    print(f"ADJOINT_LGMRES hex13_dirichlet_s0: (0, 1.0) {lifted['nstep']} | (1, 1.0) {one['nstep']} n_aug {one['n_aug']} | (2, 1.0) "
          f"{two['nstep']} n_aug {two['n_aug']} | ratio {one['nstep'] / lifted['nstep']:.2f}")
    assert lifted["stop"] == one["stop"] == two["stop"] == "tolerance"
    assert one["nstep"] < lifted["nstep"]
    for augment, out in ((0, lifted), (1, one), (2, two)):
        assert out["n_cycles"] >= 3 and (out["n_aug"] > 0) == (augment > 0) and out["n_aug"] <= augment * (out["n_cycles"] - 1)
        _against_restatement("hex13_dirichlet_s0", case, dev, out, augment, 1.0)


# ------------------------------------------------------------------------------------------------------------- 5. the launch tolerance
@pytest.mark.parametrize("name", ["hex13_mixed_s1", "hex26_dirichlet_s0"])
def test_accuracy_at_the_launch_tolerance(name, dev):
    case = LIN[name]
    P = _bound_case(case, dev)[0]
    plain, one = _dev_run(case, dev, 0, 0.5, 1e-8, 500), _dev_run(case, dev, 1, 1.0, 1e-8, 500)
    e0, e1 = P.error(plain["result"]), P.error(one["result"])
    print(f"ADJOINT_LGMRES {name} eps 1e-8 budget 500 m {M}: (0, 0.5) {plain['nstep']} products, {plain['stop']}, lowest "
          f"{plain['lowest']:.2e}, error {e0:.2e} | (1, 1.0) {one['nstep']} products, {one['stop']}, lowest {one['lowest']:.2e}, n_aug "
          f"{one['n_aug']}, error {e1:.2e}")
    assert e0 > 1e-2, e0
    assert e1 < 1e-3, e1
    for out in (plain, one):
        assert out["stop"] in ("stagnation", "tolerance") and out["nstep"] < 500, (out["stop"], out["nstep"])


# ------------------------------------------------------------------------------------------------------------- 6. handle reuse
def test_the_ring_carries_nothing_from_one_solve_into_the_next(dev):
    case = LIN["hex13_mixed_s1"]
    P, fmap, H, g, handle = _bound_case(case, dev)
    g2 = 0.5 * torch.randn(g.shape, generator=torch.Generator().manual_seed(7)).to(dev)
    chain = hr.Reused("gmres with kept corrections", lambda: _aug(fmap, dev, augment=2))
    a = chain.link("A: grad, augment 2, stall 1.0", lambda sv: sv.solve_adjoint(fmap, H, g, EPS, BUDGET, lin=handle, stall=1.0))
    b = chain.link("B: another grad, augment 2, stall 1.0", lambda sv: sv.solve_adjoint(fmap, H, g2, EPS, BUDGET, lin=handle, stall=1.0))
    c = chain.link("C: grad, augment 1, eps 1e-8", lambda sv: sv.solve_adjoint(fmap, H, g, 1e-8, 300, lin=handle, augment=1, stall=1.0))
    d = chain.link("D: another grad, no options", lambda sv: sv.solve_adjoint(fmap, H, g2, EPS, BUDGET, lin=handle, augment=0))
    assert chain.pairs == 3 and a["n_aug"] > 0 and b["n_aug"] > 0 and c["n_aug"] > 0 and d["n_aug"] == 0
    plain = pkg("engine").DeviceGmres(fmap.plan.N * 10, dev, M)
    _same(d, plain.solve_adjoint(fmap, H, g2, EPS, BUDGET, lin=handle))   # after three augmented solves: DeviceGmres's bits
    plain.close()
    chain.close()


# ------------------------------------------------------------------------------------------------------------- 7. the model
KEYS = dict(bw_solver="gmres", bw_gmres_m=10, bw_gmres_augment=1, bw_gmres_stall=1.0)


def _lin_kw(name, linearize):
    kw = {}
    if linearize:
        kw["bw_linearize"] = True
        if CASES[name] == "mixed":
            kw["lin_neumann"] = "stored"
    return kw


def _step(net, mesh, dev):
    u, ld = net(mesh.to(dev))
    (ld["residual_loss"] + ld["encoder_loss"] + ld["autoencoder_loss"]).backward()
    return {k: p.grad.clone() for k, p in net.named_parameters()}


@pytest.mark.parametrize("linearize", [False, True])
@pytest.mark.parametrize("name", ["hex13_mixed_s1", "hex13_dirichlet_s0"])
def test_training_step_with_the_keys(name, linearize, dev):
    sd = load_weights(CASES[name])
    T = np.load(os.path.join(GOLDEN, "grad_truth_fp64.npz"))
    mesh = _draw(name, 0)
    net = _model(sd, dev, fw_tol=1e-7, fw_thres=600, **KEYS, **_lin_kw(name, linearize)).train()
    got = _step(net, mesh, dev)
    bw = net.deqdss.last_backward
    assert type(net.deqdss._bw_gmres) is pkg("engine").DeviceGmresAug and net.deqdss._bw_gmres_key[1:] == (10, 1, "aug")
    assert bw["n_aug"] > 0 and bw["augment"] == 1 and bw["stop"] in ("tolerance", "stagnation") and bw["threshold"] == 400, bw["stop"]
    want = {k: torch.from_numpy(T[f"{name}/0/{k}"]) for k in got}
    scale = max(float(t.norm()) for t in want.values())
    e, k = _worst(got, want, scale)
    print(f"ADJOINT_LGMRES training {name} linearize={linearize}: worst-tensor gradient error vs fp64 truth {e:.2e} ({k}); {bw['nstep']} "
          f"products, {bw['n_cycles']} cycles, n_aug {bw['n_aug']}, {bw['stop']}, lowest {bw['lowest']:.2e}")
    assert e < 1e-2, (k, e)
    # the two keys at their defaults: the objects and the bits of a model without them
    base_kw = dict(fw_tol=1e-7, fw_thres=600, bw_solver="gmres", bw_gmres_m=10, **_lin_kw(name, linearize))
    without = _model(sd, dev, **base_kw).train()
    g0 = _step(without, mesh, dev)
    with_defaults = _model(sd, dev, bw_gmres_augment=0, bw_gmres_stall=0.5, **base_kw).train()
    g1 = _step(with_defaults, mesh, dev)
    assert type(with_defaults.deqdss._bw_gmres) is pkg("engine").DeviceGmres and "n_aug" not in with_defaults.deqdss.last_backward
    assert all(torch.equal(g0[k], g1[k]) for k in g0)
    _same(without.deqdss.last_backward, with_defaults.deqdss.last_backward)


@pytest.mark.parametrize("family", ["dirichlet", "mixed"])
def test_replicas_with_the_keys_solve_one_after_the_other(family, dev):
    """DataParallel(replicas=2) with the keys, ``bw_gmres_lockstep`` set or not: no lockstep route, each replica's adjoint solve is the
    single-batch one with kept corrections."""
    loader, nat = pkg("loader"), pkg("_native")
    names = [("hex13_dirichlet_s0", 0), ("original_dirichlet_s0", 0)] if family == "dirichlet" else [("hex13_mixed_s1", 0), ("hex13_mixed_s1", 1)]
    sd = load_weights(family)
    meshes = [_draw(n, d) for n, d in names]
    kw = dict(fw_tol=1e-7, fw_thres=600, bw_linearize=True, **KEYS)
    if family == "mixed":
        kw.update(lin_neumann="stored", bw_gmres_lockstep=True)   # the lockstep GMRES takes no options: the key does not apply
    net = _model(sd, dev, **kw).train()
    wrapped = loader.DataParallel(net, replicas=2).to(dev)
    us, ld = wrapped(meshes)
    nat.prof_enable(True)
    nat.prof_collect()
    (ld["residual_loss"] + ld["encoder_loss"] + ld["autoencoder_loss"]).sum().backward()
    ran = nat.prof_collect()
    nat.prof_enable(False)
    assert "k_vjp_lin_batch" not in ran and "k_lg_check" in ran and "k_ag_check" not in ran, sorted(ran)
    assert "k_lg_shift" in ran and "k_lg_combine" in ran and "k_lg_norm" in ran
    bws = net.deqdss.last_backward
    assert len(bws) == 2 and all(o["stop"] in ("tolerance", "stagnation") and o["n_aug"] > 0 for o in bws)
    one = _model(sd, dev, **kw).train()
    _step(one, meshes[1], dev)
    hr.same_out(one.deqdss.last_backward, bws[1], "replica 1 against the single-batch step")
