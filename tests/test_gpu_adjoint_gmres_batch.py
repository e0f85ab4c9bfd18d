"""GPU: the lockstep form of the restarted GMRES adjoint solve (csrc/krylov.hip ``psignn_gmres_solve_adjoint_lin_batch``,
``engine.gmres_solve_adjoint_batch``) and the replica training route built on it (model config keys ``bw_solver = "gmres"`` +
``bw_gmres_lockstep = True``).

Contract under test: for every replica of a shard ``result``, ``nstep`` (products), ``n_cycles``, ``stop``, ``n_reorth``, ``lowest``,
``lowest_abs`` and both traces of the batched solve are bit-identical to ``DeviceGmres.solve_adjoint(..., lin=)`` with the same
handle on that replica alone, whatever ``poll_every``.  The shards are those of tests/test_gpu_adjoint_batch.py (``_shard``): ragged
hexagon meshes, H* from the batched forward solve at 1e-5 / 300, seeded Gaussian grads, the GMRES handles made with ``shard_elems`` =
the shard's total.

Replica step: every ``last_backward[r]`` against a single-batch model bit by bit; the summed gradient against the sum of the
single-batch gradients within 1e-5 relative (the bound of test_replicas_solve_one_after_the_other); each replica's gradient against
the stored float64 truth under the criterion of tests/test_gpu_training.py::test_training_step_gradients (every run within 1e-2, the
mean of the worst-tensor errors of a fixture's draws within max(5e-3, 1.25 x the reference path's mean))."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from conftest import CASES, load_weights, pkg
from test_gpu_adjoint_batch import REPLICAS, _draw, _shard
from test_gpu_training import _model, _worst

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
FIELDS = ("nstep", "n_cycles", "stop", "n_reorth", "lowest", "lowest_abs", "rel_trace", "abs_trace")
SMALL = (10, 1e-6, 120)     # (m, eps, budget): several cycles per mesh, both stops over the shard
TRAIN = (50, 1e-8, 500)     # the training configuration (bw_gmres_m, bw_tol, bw_thres)


@functools.lru_cache(maxsize=None)
def _gshard(mixed):
    """The shard of test_gpu_adjoint_batch._shard (computed once per family, left unchanged), without its Broyden adjoint solvers."""
    S = _shard(torch.device("cuda:0"), mixed)
    for sv in S.pop("solvers"):
        sv.close()
    return S


def _handles(S, m, shard_elems="total"):
    eng = pkg("engine")
    tot = S["total"] if shard_elems == "total" else shard_elems
    return [eng.DeviceGmres(f.plan.N * 10, f.plan.device, m, shard_elems=tot) for f in S["fmaps"]]


def _same(a, b, what=""):
    for k in FIELDS:
        assert a[k] == b[k], (what, k, a[k] if not isinstance(a[k], list) else "trace", b[k] if not isinstance(b[k], list) else "trace")
    assert torch.equal(a["result"], b["result"]), what


def _singles(S, handles, eps, budget):
    return [sv.solve_adjoint(f, h, g, eps, budget, lin=l) for sv, f, h, g, l in zip(handles, S["fmaps"], S["H"], S["grads"], S["lins"])]


@pytest.mark.parametrize("family", ["dirichlet", "mixed"])
def test_batched_gmres_bit_identical_on_ragged_shard(family, dev):
    """Single solves with the same handles first, then the batched solve: every field of the contract and the result's bits, at
    (m, eps, budget) = (10, 1e-6, 120) for two poll intervals and at the training configuration (50, 1e-8, 500).  The CPU restatement
    (tests/adjoint_gmres_ref.py on the oracle VJP) gives at (10, 1e-6, 120): dirichlet cycles 7 / 10 / 8 / 4 / 9 / 4, products
    64 / 98 / 77 / 33 / 88 / 33, four tolerance and two stagnation stops; mixed cycles 8 / 4 / 6 / 4 / 11, products 77 / 33 / 55 / 33 /
    110, two tolerance and three stagnation stops -- the GPU counts may differ by a cycle."""
    eng, nat = pkg("engine"), pkg("_native")
    S = _gshard(family == "mixed")
    m, eps, budget = SMALL
    handles = _handles(S, m)
    assert eng.gmres_adjoint_batchable(handles, S["lins"])
    single = _singles(S, handles, eps, budget)
    nat.prof_enable(True)
    nat.prof_collect()
    outs = eng.gmres_solve_adjoint_batch(handles, S["lins"], S["grads"], eps, budget)
    ran = nat.prof_collect()
    nat.prof_enable(False)
    print(f"ADJOINT_GMRES_BATCH {family} {SMALL}: cycles single {[o['n_cycles'] for o in single]} batched {[o['n_cycles'] for o in outs]}; "
          f"products {[o['nstep'] for o in outs]}; stops {[o['stop'] for o in outs]}; lowest {['%.2e' % o['lowest'] for o in outs]}; "
          f"launches k_vjp_lin_batch {ran.get('k_vjp_lin_batch', (0,))[0]} k_gm_finish_batch {ran.get('k_gm_finish_batch', (0,))[0]}")
    for r, (a, b) in enumerate(zip(single, outs)):
        _same(a, b, f"replica {r} poll 8")
    # the route: batched kernels only, one product launch for the whole shard
    assert "k_vjp_lin_batch" in ran and "k_ag_check_batch" in ran, sorted(ran)
    for name in ("k_vjp_lin", "k_vjp_lin_mixed", "k_ag_check", "k_gm_finish"):
        assert name not in ran, (name, sorted(ran))
    nsteps = [o["nstep"] for o in outs]
    assert max(nsteps) <= ran["k_vjp_lin_batch"][0] < sum(nsteps), (nsteps, ran["k_vjp_lin_batch"][0])
    assert ran["k_gm_finish_batch"][0] <= ran["k_vjp_lin_batch"][0]
    outs3 = eng.gmres_solve_adjoint_batch(handles, S["lins"], S["grads"], eps, budget, poll_every=3)
    for r, (a, b) in enumerate(zip(single, outs3)):
        _same(a, b, f"replica {r} poll 3")
    # the shard really is ragged in cycles, and both stops occur (else the gates above could hide a broken one)
    assert len({o["n_cycles"] for o in outs}) >= 3, [o["n_cycles"] for o in outs]
    stops = {o["stop"] for o in outs}
    assert "tolerance" in stops and "stagnation" in stops, [o["stop"] for o in outs]
    for sv in handles:
        sv.close()
    # the training configuration
    m, eps, budget = TRAIN
    handles = _handles(S, m)
    single = _singles(S, handles, eps, budget)
    outs = eng.gmres_solve_adjoint_batch(handles, S["lins"], S["grads"], eps, budget)
    print(f"ADJOINT_GMRES_BATCH {family} {TRAIN}: cycles {[o['n_cycles'] for o in outs]}; products {[o['nstep'] for o in outs]}; "
          f"stops {[o['stop'] for o in outs]}")
    for r, (a, b) in enumerate(zip(single, outs)):
        _same(a, b, f"replica {r} training configuration")
    for sv in handles:
        sv.close()


def test_batched_gmres_run_to_run(dev):
    eng = pkg("engine")
    S = _gshard(False)
    m, eps, budget = SMALL
    handles = _handles(S, m)
    a = eng.gmres_solve_adjoint_batch(handles, S["lins"], S["grads"], eps, budget)
    b = eng.gmres_solve_adjoint_batch(handles, S["lins"], S["grads"], eps, budget)
    for r, (x, y) in enumerate(zip(a, b)):
        _same(x, y, f"replica {r}")
    for sv in handles:
        sv.close()


def test_batched_gmres_refusals(dev):
    """Shards the lockstep does not take: gmres_adjoint_batchable is False and the batched call raises with nothing launched."""
    eng, nat = pkg("engine"), pkg("_native")
    Dr, Mx = _gshard(False), _gshard(True)
    m, eps, budget = SMALL
    f0, f1, mf = Dr["fmaps"][0], Dr["fmaps"][1], Mx["fmaps"][0]
    tot = Dr["total"]
    mk = lambda f, mm=m, shard=tot: eng.DeviceGmres(f.plan.N * 10, f.plan.device, mm, shard_elems=shard)
    s0, s1, sm = mk(f0), mk(f1), mk(mf)
    l0, l1 = Dr["lins"][0], Dr["lins"][1]
    g0, g1, gm = Dr["grads"][0], Dr["grads"][1], Mx["grads"][0]
    # a handle made without shard_elems has another width only where its own length is on the other side of the width switch
    # (3 * 2^18 elements) from the shard's; this shard is below it, so the odd handle out is one with another restart length
    assert tot < 3 << 18
    other_m = mk(f1, mm=m + 1)
    wrong_len = mk(f0)          # made for mesh 0's length, paired with mesh 1's linearisation
    unbuilt = eng.Linearization(f1)
    direct = mf.linearize_p(mf.to_plan(Mx["H"][0]), neumann="direct")
    assert not direct.neumann_stored
    # n_layers = 2: the handle's map carries a two-layer weight pack (the batched solve runs single-layer blocks)
    sd2 = pkg("model_psignn").ModelPSIGNN(dict(latent_dim=10, n_layers=2)).state_dict()
    f0_two = eng.FixedPointMap(f0.plan, eng.PackedWeights(sd2, dev), f0.h0, f0.prb, None)
    assert f0_two.weights.n_layers == 2
    two = f0.linearize_p(f0.to_plan(Dr["H"][0]))
    two.fmap = f0_two
    cases = {
        "another restart length": ([s0, other_m], [l0, l1], [g0, g1]),
        "handle of another length than its plan": ([s0, wrong_len], [l0, l1], [g0, g1]),
        "unbuilt linearisation": ([s0, s1], [l0, unbuilt], [g0, g1]),
        "mixed handle, neumann direct": ([sm], [direct], [gm]),
        "both families": ([s0, sm], [l0, Mx["lins"][0]], [g0, gm]),
        "n_layers = 2": ([s0], [two], [g0]),
    }
    assert eng.gmres_adjoint_batchable([s0, s1], [l0, l1]) and eng.gmres_adjoint_batchable([sm], [Mx["lins"][0]])
    nat.prof_enable(True)
    for what, (svs, lins, grads) in cases.items():
        assert not eng.gmres_adjoint_batchable(svs, lins), what
        nat.prof_collect()
        with pytest.raises(nat.NativeError):
            eng.gmres_solve_adjoint_batch(svs, lins, grads, eps, budget)
        assert nat.prof_collect() == {}, what
    nat.prof_enable(False)
    for o in (s0, s1, sm, other_m, wrong_len, unbuilt, direct, two):
        o.close()


# ---- training step of three replicas ------------------------------------------------------------------------------------
def _params_grad(net):
    return {k: p.grad.clone() for k, p in net.named_parameters()}


@pytest.mark.parametrize("family", ["dirichlet", "mixed"])
def test_replica_training_step_with_lockstep_gmres(family, dev):
    """DataParallel(net, replicas=3) on the REPLICAS meshes with bw_solver = "gmres", bw_gmres_lockstep = True, bw_linearize = True
    (mixed: lin_neumann = "stored").  The shard is far below the 3 * 2^18-element width switch, so the replica handles (sized for
    the shard) and the single-batch model's handle (sized for itself) both take the 4-float kernels: the bits must agree."""
    loader, nat = pkg("loader"), pkg("_native")
    reps = REPLICAS[family]
    sd = load_weights(family)
    meshes = [_draw(n, d) for n, d in reps]
    kw = dict(fw_tol=1e-7, fw_thres=600, bw_solver="gmres", bw_linearize=True)
    if family == "mixed":
        kw["lin_neumann"] = "stored"
    net = _model(sd, dev, bw_gmres_lockstep=True, **kw).train()
    wrapped = loader.DataParallel(net, replicas=3).to(dev)
    us, ld = wrapped(meshes)
    assert ld["residual_loss"].shape == (3,)
    assert sum(m.num_nodes for m in meshes) * 10 < 3 << 18
    per = ld["residual_loss"] + ld["encoder_loss"] + ld["autoencoder_loss"]
    nat.prof_enable(True)
    nat.prof_collect()
    per.sum().backward(retain_graph=True)
    ran = nat.prof_collect()
    nat.prof_enable(False)
    assert "k_vjp_lin_batch" in ran and "k_ag_check_batch" in ran and "k_ag_check" not in ran and "k_xnext" not in ran, sorted(ran)
    bws = list(net.deqdss.last_backward)
    assert len(bws) == 3 and all(o["stop"] in ("tolerance", "stagnation") for o in bws), [o["stop"] for o in bws]
    assert all(o["eps"] == 1e-7 and o["threshold"] == 400 for o in bws)
    got = _params_grad(net)
    # the single-batch route on each replica's batch
    singles = []
    for r, m in enumerate(meshes):
        one = _model(sd, dev, **kw).train()
        u, l1 = one(m.to(dev))
        (l1["residual_loss"] + l1["encoder_loss"] + l1["autoencoder_loss"]).backward()
        _same(one.deqdss.last_backward, bws[r], f"replica {r}")
        singles.append(_params_grad(one))
    for k in got:
        want = sum(s[k].double() for s in singles)
        assert float((got[k].double() - want).norm()) <= 1e-5 * max(float(want.norm()), 1e-30), k
    # each replica's own gradient (the other replicas' losses left out: their adjoint systems have a zero right-hand side) against
    # the float64 truth, criterion of test_training_step_gradients
    T = np.load(os.path.join(GOLDEN, "grad_truth_fp64.npz"))
    bands = json.load(open(os.path.join(GOLDEN, "grad_error_band.json")))
    errs = {}
    for r, (name, draw) in enumerate(reps):
        net.zero_grad()
        per[r].backward(retain_graph=r + 1 < len(reps))
        got_r = {k: p.grad for k, p in net.named_parameters()}
        want = {k: torch.from_numpy(T[f"{name}/{draw}/{k}"]) for k in got_r}
        scale = max(float(t.norm()) for t in want.values())
        e, k = _worst(got_r, want, scale)
        errs.setdefault(name, []).append(e)
        assert e < 1e-2, (name, draw, k, e)
    for name, es in errs.items():
        print(f"ADJOINT_GMRES_BATCH training {name}: worst-tensor gradient errors vs fp64 truth {['%.2e' % e for e in es]}, "
              f"mean {np.mean(es):.2e}; reference path mean {bands[name]['mean']:.2e}")
        assert np.mean(es) <= max(5e-3, 1.25 * bands[name]["mean"]), (name, es, bands[name]["mean"])


def test_replica_step_falls_back_on_an_untiled_plan(dev):
    """Key true, one replica on an untiled plan: lockstep_applies says no on the host, the replicas are solved one after the other
    (k_ag_check runs, no batched kernel) and the gradients are those of the same step with the key false."""
    eng, nat = pkg("engine"), pkg("_native")
    sd = load_weights("dirichlet")
    kw = dict(fw_tol=1e-7, fw_thres=600, bw_solver="gmres", bw_linearize=True)
    grads = {}
    for key in (True, False):
        mds = [_draw(n, d).to(dev) for n, d in REPLICAS["dirichlet"][:2]]
        flat = eng.MeshPlan(mds[1], tile_target=-1)
        assert not flat.tiled
        eng.plan_for(mds[1])                                              # the cache key of this batch ...
        mds[1]._psignn_plan = (mds[1]._psignn_plan[0], flat)              # ... now holds the untiled plan
        net = _model(sd, dev, bw_gmres_lockstep=key, **kw).train()
        fmaps = [net.deqdss.f.bind(net.autoencoder.encoder(b.x).detach(), b) for b in mds]
        assert fmaps[0].plan.tiled and fmaps[1].plan is flat and not net.deqdss.lockstep_applies(fmaps)
        us, ld = net(mds)
        nat.prof_enable(True)
        nat.prof_collect()
        (ld["residual_loss"] + ld["encoder_loss"] + ld["autoencoder_loss"]).sum().backward()
        ran = nat.prof_collect()
        nat.prof_enable(False)
        assert "k_ag_check" in ran and "k_ag_check_batch" not in ran and "k_vjp_lin_batch" not in ran, sorted(ran)
        assert len(net.deqdss.last_backward) == 2 and all("n_cycles" in o for o in net.deqdss.last_backward)
        grads[key] = _params_grad(net)
    assert all(torch.equal(grads[True][k], grads[False][k]) for k in grads[True])
