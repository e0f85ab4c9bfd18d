"""Lockstep Anderson / Picard solves of a shard of meshes (engine.anderson_solve_batch / picard_solve_batch, utilities.solver.
anderson_batch / forward_iteration_batch, the model key fp_lockstep) on the GPU.

Every equality here is bitwise -- ``torch.equal`` on tensors, ``==`` on traces and counters: the lockstep solve runs the arithmetic of
the single-mesh route in the same order (same block -> element mapping, same partial-sum shapes, the same tile body for f), so no
tolerance is involved.  Shards are those of tests/test_gpu_adjoint_batch.py::_shard: ``make_hex_problem(n, seed=s, mixed=...)`` with
sizes (10, 13, 11, 26, 12, 40) for dirichlet and (9, 40, 13, 58, 26) for mixed on the stored checkpoints -- 271 to 10 267 nodes per
mesh, ragged in tiles and in vector blocks."""
import functools

import pytest
import torch

import limit_graphs as lg
import recurrences as rc
from conftest import load_weights, pkg

pytestmark = pytest.mark.gpu

SIZES = {False: (10, 13, 11, 26, 12, 40), True: (9, 40, 13, 58, 26)}
FP_KERNELS = ("k_and_gram", "k_and_solve", "k_and_mix", "k_fp_norms", "k_and_check")
FIELDS = ("n_iter", "nstep", "lowest", "lowest_abs", "stop_reason", "rel_trace", "abs_trace", "low_idx")


def _mod(mixed):
    return pkg("mixed") if mixed else pkg("model_psignn")


@functools.lru_cache(maxsize=None)
def _shard(mixed):
    """Meshes, device batches and bound maps of one family's shard (built once per session, never modified)."""
    data = pkg("data")
    dev = torch.device("cuda:0")
    sd = load_weights("mixed" if mixed else "dirichlet")
    net = _mod(mixed).ModelPSIGNN(dict(latent_dim=10, n_layers=1))
    net.load_state_dict(sd)
    net = net.to(dev).eval()
    meshes = [data.make_hex_problem(n, seed=s, mixed=mixed) for s, n in enumerate(SIZES[mixed])]
    mds = [m.to(dev) for m in meshes]
    with torch.no_grad():
        fmaps = [net.deqdss.f.bind(net.autoencoder.encoder(md.x), md) for md in mds]
    assert all(f.plan.tiled and bool(f.plan.mixed) == mixed for f in fmaps)
    total = sum(f.plan.N for f in fmaps) * 10
    assert total < 3 << 18          # the shard's handles and a mesh's own handle both take the 4-float kernels
    return dict(sd=sd, meshes=meshes, mds=mds, fmaps=fmaps, total=total)


def _profiled(fn):
    nat = pkg("_native")
    nat.prof_enable(True)
    nat.prof_collect()
    try:
        out = fn()
        ran = nat.prof_collect()
    finally:
        nat.prof_enable(False)
    return out, ran


def _floats(tr):
    return [float(t) for t in tr]


def _stepwise_anderson(it, fmap, T, eps, lam=1e-4, beta=1.0, stop_mode="rel", F=None):
    """The stepwise API on one handle around fmap.fp: what ``solver.anderson`` does, without its poll.  Result in plan order."""
    F = F or fmap.fp
    xp = fmap.to_plan(fmap.h0)
    f0 = F(xp)
    f1 = F(f0)
    it.anderson_begin(xp, f0, f1, lam, beta, stop_mode == "abs")
    for _ in range(2, T):
        it.anderson_update(F(it.anderson_next(xp)), eps)
    return it.finish(xp)


def _stepwise_picard(it, fmap, T, eps):
    xp = fmap.to_plan(fmap.h0)
    it.picard_begin(xp)
    for _ in range(T + 1):
        it.picard_update(fmap.fp(it.picard_current(xp)), eps)
    return it.finish(xp)


def _same_as_stepwise(fmap, step, got, where):
    assert torch.isfinite(got["result"]).all(), where
    assert torch.equal(fmap.from_plan(step["result"]), got["result"]), (where, "result")
    for k in FIELDS:
        assert step[k] == got[k], (where, k, step[k], got[k])


# ------------------------------------------------------------------------------------------------ 1. the public single-mesh solvers
@pytest.mark.parametrize("mixed", [False, True])
def test_equal_to_the_public_solvers(mixed, dev):
    """shard_elems = the real total (4 floats per lane, as a mesh's own handle): ``anderson_batch`` at m = 2, threshold 40, eps = 0
    against ``solver.anderson`` mesh by mesh, ``forward_iteration_batch`` at eps 1e-5, threshold 60 against
    ``solver.forward_iteration``."""
    slv = pkg("utilities.solver")
    S = _shard(mixed)
    outs = slv.anderson_batch(S["fmaps"], m=2, threshold=40, eps=0.0)
    for i, (f, o) in enumerate(zip(S["fmaps"], outs)):
        ref = slv.anderson(f, f.h0, m=2, lam=1e-4, threshold=40, eps=0.0, keep_trace=False)
        assert torch.equal(ref["result"], o["result"]), i
        for k in ("nstep", "lowest", "rel_trace", "abs_trace"):
            assert ref[k] == o[k], (i, k)
        assert len(o["rel_trace"]) == 38 and o["xest_trace"].keep_trace is False and o["prot_break"] is False
    outs = slv.forward_iteration_batch(S["fmaps"], eps=1e-5, threshold=60)
    for i, (f, o) in enumerate(zip(S["fmaps"], outs)):
        ref = slv.forward_iteration(f, f.h0, eps=1e-5, threshold=60, keep_trace=False)
        assert torch.equal(ref["result"], o["result"]), i
        assert ref["nstep"] == o["nstep"] and float(ref["lowest"]) == float(o["lowest"]), i
        assert _floats(ref["rel_trace"]) == _floats(o["rel_trace"]) and _floats(ref["abs_trace"]) == _floats(o["abs_trace"]), i
        assert o["xest_trace"].keep_trace is False


# ------------------------------------------------------------------------------------------------ 2. the stepwise API, 16 floats per lane
@pytest.mark.parametrize("stop_mode", ["rel", "abs"])
@pytest.mark.parametrize("beta", [1.0, 0.6])
@pytest.mark.parametrize("m", [2, 3, 8])
@pytest.mark.parametrize("mixed", [False, True])
def test_equal_to_the_stepwise_api_at_16_floats_per_lane(mixed, m, beta, stop_mode, dev):
    """shard_elems = 2^20 forces the 16-float kernels on these small meshes: every mesh ends in a partial block.  12 loop passes
    (threshold 14, eps 0); the same handles are driven step by step first, with a recorder around fmap.fp whose points and values
    must satisfy the Anderson recurrences in float64, then solved in lockstep."""
    eng = pkg("engine")
    S = _shard(mixed)
    T = 14
    iters = [eng.DeviceFixedPointIter(f.plan.N * 10, dev, m=m, threshold=T, shard_elems=1 << 20) for f in S["fmaps"]]
    try:
        steps = []
        for i, (it, f) in enumerate(zip(iters, S["fmaps"])):
            rec = rc.Recorder(f.fp)
            st = _stepwise_anderson(it, f, T, 0.0, beta=beta, stop_mode=stop_mode, F=rec)
            out = dict(st, lowest=st["lowest_abs"] if stop_mode == "abs" else st["lowest"])
            n = rc.check_anderson(rec.P, rec.R, out, m, 1e-4, beta, T, 0.0, stop_mode, where=f"mesh {i} m={m} beta={beta} {stop_mode}")
            assert n == T - 2
            steps.append(st)
        assert eng.fpiter_batchable(iters, S["fmaps"])
        got = eng.anderson_solve_batch(iters, S["fmaps"], 0.0, lam=1e-4, beta=beta, stop_mode=stop_mode)
        for i, (f, st, o) in enumerate(zip(S["fmaps"], steps, got)):
            _same_as_stepwise(f, st, o, (mixed, m, beta, stop_mode, i))
            assert len(o["low_idx"]) == T - 2
    finally:
        for it in iters:
            it.close()


# ------------------------------------------------------------------------------------------------ 3. staggered stops, poll_every
def test_staggered_stops_do_not_depend_on_poll_every(dev):
    """eps_mid = 1.02 x mesh 0's rel_trace[30] of the eps = 0 reference runs (threshold 80), the construction of
    tests/test_gpu_parity.py::test_forward_iteration_anderson_newton.  On the CPU oracle (``oracle.anderson`` on the same six
    meshes, float32) step 30 gives the loop passes [31, 64, 78, 43, 78, 54]: mesh 0 stops first, two meshes run to the threshold.
    The staggering is asserted on the single-mesh reference runs, then the lockstep solve at poll_every 1, 5 and 8 must equal them
    mesh by mesh -- result, nstep and the padded traces.  Picard likewise with eps between the smallest and the largest final rel
    of the reference runs at threshold 60 (oracle: 2.2e-4 .. 1.07e-3, no mesh converges to 1e-5 in 60 passes)."""
    slv = pkg("utilities.solver")
    fmaps = _shard(False)["fmaps"]
    T = 80
    free = [slv.anderson(f, f.h0, threshold=T, eps=0.0, keep_trace=False) for f in fmaps]
    eps_mid = 1.02 * free[0]["rel_trace"][30]
    n_iter = [next((i + 1 for i, r in enumerate(o["rel_trace"]) if r < eps_mid), T - 2) for o in free]
    print("FPBATCH anderson eps_mid", eps_mid, "loop passes", n_iter)
    assert min(n_iter) < T - 2 and len(set(n_iter)) >= 2, n_iter
    refs = [slv.anderson(f, f.h0, threshold=T, eps=eps_mid, keep_trace=False) for f in fmaps]
    for pe in (1, 5, 8):
        for i, (ref, o) in enumerate(zip(refs, slv.anderson_batch(fmaps, threshold=T, eps=eps_mid, poll_every=pe))):
            assert torch.equal(ref["result"], o["result"]), (pe, i)
            for k in ("nstep", "lowest", "rel_trace", "abs_trace"):
                assert ref[k] == o[k], (pe, i, k)
            assert len(o["rel_trace"]) == T - 2
    # Picard
    T = 60
    free = [slv.forward_iteration(f, f.h0, eps=1e-5, threshold=T, keep_trace=False) for f in fmaps]
    last = [float(o["rel_trace"][-1]) for o in free]
    eps_p = (min(last) * max(last)) ** 0.5
    assert min(last) < eps_p < max(last), last
    refs = [slv.forward_iteration(f, f.h0, eps=eps_p, threshold=T, keep_trace=False) for f in fmaps]
    nsteps = [o["nstep"] for o in refs]
    print("FPBATCH picard eps", eps_p, "nstep", nsteps)
    assert min(nsteps) < T and len(set(nsteps)) >= 2, nsteps
    for pe in (1, 5, 8):
        for i, (ref, o) in enumerate(zip(refs, slv.forward_iteration_batch(fmaps, eps=eps_p, threshold=T, poll_every=pe))):
            assert torch.equal(ref["result"], o["result"]), (pe, i)
            assert ref["nstep"] == o["nstep"] and float(ref["lowest"]) == float(o["lowest"]), (pe, i)
            assert _floats(ref["rel_trace"]) == _floats(o["rel_trace"]) and _floats(ref["abs_trace"]) == _floats(o["abs_trace"]), (pe, i)


# ------------------------------------------------------------------------------------------------ 4. launch record
def test_launches_per_iteration_do_not_depend_on_the_shard(dev):
    """eps = 0, threshold T = 14: a shard of one mesh and the shard of six record the same launches -- T - 2 of each Anderson
    kernel and T tile-f launches (two initial evaluations, one per loop pass)."""
    slv = pkg("utilities.solver")
    fmaps = _shard(False)["fmaps"]
    T = 14
    for shard in (fmaps[:1], fmaps):
        _, ran = _profiled(lambda: slv.anderson_batch(shard, threshold=T, eps=0.0))
        for name in FP_KERNELS:
            assert ran.get(name, (0,))[0] == T - 2, (len(shard), name, ran.get(name))
        assert ran.get("k_f_tile", (0,))[0] == T, (len(shard), ran.get("k_f_tile"))
        assert set(ran) == set(FP_KERNELS) | {"k_f_tile"}, sorted(ran)
    _, ran = _profiled(lambda: slv.forward_iteration_batch(fmaps, eps=0.0, threshold=T))
    assert ran["k_fp_norms"][0] == ran["k_picard_check"][0] == ran["k_f_tile"][0] == T + 1, ran


# ------------------------------------------------------------------------------------------------ 5. largest LDS request, other widths
def _random(d, mixed, L=1, seed=5):
    """Seeded random blocks, the recipe of tests/test_gpu_latent_width.py::_random."""
    torch.manual_seed(seed)
    net = _mod(mixed).ModelPSIGNN(dict(latent_dim=d, n_layers=L))
    for p in net.parameters():
        if p.dim() == 1:
            torch.nn.init.normal_(p, std=0.1)
    return {k: v.detach().clone() for k, v in net.state_dict().items()}


def _maps(meshes, tile_targets, d, mixed, dev, L=1):
    """Maps of ``meshes`` on one packed weight buffer of width d, h0 = 0.3 x seeded Gaussian (as the limit test builds its map)."""
    eng = pkg("engine")
    w = eng.PackedWeights(_random(d, mixed, L), dev)
    gen = torch.Generator().manual_seed(21)
    fmaps = []
    for mesh, tt in zip(meshes, tile_targets):
        md = mesh.to(dev)
        h0 = 0.3 * torch.randn(mesh.num_nodes, d, generator=gen)
        fmaps.append(eng.FixedPointMap(eng.MeshPlan(md, tile_target=tt), w, h0.to(dev), md.prb_data, getattr(md, "unit_normal_vector", None)))
    return fmaps


@pytest.mark.parametrize("case", ["halo512_d16", "mixed_d8"])
def test_other_widths_and_the_largest_lds_request(case, dev):
    """Width 16, dirichlet: the ``halo512`` limit graph (768 LDS rows x 128 B = 98 304 B of dynamic LDS, above the 64 KiB default)
    between two small meshes.  Width 8, mixed: three meshes.  Anderson (m = 3, 8 loop passes) and Picard (6 passes) in lockstep
    against the stepwise API on the same handles."""
    eng, data = pkg("engine"), pkg("data")
    if case == "halo512_d16":
        d, mixed = 16, False
        c = lg.build("halo512", False)
        meshes = [data.make_hex_problem(10, seed=0), c.mesh, data.make_hex_problem(13, seed=1)]
        fmaps = _maps(meshes, [0, c.tile_target, 0], d, mixed, dev)
        assert c.tiled and fmaps[1].plan.tiled and fmaps[1].plan.max_tile_rows == c.max_rows == 768
    else:
        d, mixed = 8, True
        fmaps = _maps([data.make_hex_problem(n, seed=s, mixed=True) for s, n in enumerate((9, 13, 26))], [0, 0, 0], d, mixed, dev)
    assert all(f.width == d and f.plan.tiled for f in fmaps)
    total = sum(f.plan.N for f in fmaps) * d
    T = 10
    iters = [eng.DeviceFixedPointIter(f.plan.N * d, dev, m=3, threshold=T, width=d, shard_elems=total) for f in fmaps]
    try:
        steps = [_stepwise_anderson(it, f, T, 0.0) for it, f in zip(iters, fmaps)]
        for i, (f, st, o) in enumerate(zip(fmaps, steps, eng.anderson_solve_batch(iters, fmaps, 0.0))):
            _same_as_stepwise(f, st, o, (case, "anderson", i))
            assert o["n_iter"] == T - 2
    finally:
        for it in iters:
            it.close()
    iters = [eng.DeviceFixedPointIter(f.plan.N * d, dev, m=1, threshold=5, width=d, shard_elems=total) for f in fmaps]
    try:
        steps = [_stepwise_picard(it, f, 5, 0.0) for it, f in zip(iters, fmaps)]
        for i, (f, st, o) in enumerate(zip(fmaps, steps, eng.picard_solve_batch(iters, fmaps, 0.0))):
            _same_as_stepwise(f, st, o, (case, "picard", i))
            assert o["n_iter"] == 6
    finally:
        for it in iters:
            it.close()


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_launch_nothing(dev):
    """A shard that mixes families, holds an untiled plan, handles of two thresholds or two vector widths, a handle with a kept trace,
    or two-layer weights: ``NativeError`` from both solves, ``fpiter_batchable`` says no, and the launch record stays empty."""
    eng, nat, data = pkg("engine"), pkg("_native"), pkg("data")
    D, M = _shard(False), _shard(True)
    fd, fm = D["fmaps"][:2], M["fmaps"][:1]
    mk = lambda f, **kw: eng.DeviceFixedPointIter(f.plan.N * 10, dev, **dict(dict(m=2, threshold=12, shard_elems=D["total"]), **kw))
    md = D["mds"][0]
    flat = eng.FixedPointMap(eng.MeshPlan(md, tile_target=-1), fd[0].weights, fd[0].h0, md.prb_data)
    assert not flat.plan.tiled
    two = _maps([data.make_hex_problem(10, seed=0), data.make_hex_problem(13, seed=1)], [0, 0], 10, False, dev, L=2)
    assert two[0].weights.n_layers == 2
    shards = {
        "both families": (fd[:1] + fm, [mk(fd[0]), mk(fm[0])]),
        "untiled plan": ([fd[0], flat], [mk(fd[0]), mk(flat)]),
        "two thresholds": (fd, [mk(fd[0]), mk(fd[1], threshold=13)]),
        "two vector widths": (fd, [mk(fd[0]), mk(fd[1], shard_elems=1 << 20)]),
        "kept trace": (fd, [mk(fd[0]), mk(fd[1], keep_trace=True)]),
        "handle not made for a shard": (fd, [mk(fd[0]), mk(fd[1], shard_elems=None)]),
        "handle of another mesh": (fd, [mk(fd[0]), mk(fd[0])]),
        "two layers": (two, [mk(two[0]), mk(two[1])]),
    }
    for what, (fmaps, iters) in shards.items():
        def refused():
            assert not eng.fpiter_batchable(iters, fmaps), what
            with pytest.raises(nat.NativeError):
                eng.anderson_solve_batch(iters, fmaps, 0.0)
            with pytest.raises(nat.NativeError):
                eng.picard_solve_batch(iters, fmaps, 0.0)
        _, ran = _profiled(refused)
        assert ran == {}, (what, ran)
        for it in iters:
            it.close()
    # the C entry itself refuses two-layer weights and a history of one, before anything is launched
    iters = [mk(f, m=1) for f in fd]
    assert eng.fpiter_batchable(iters, fd)
    _, ran = _profiled(lambda: pytest.raises(nat.NativeError, eng.anderson_solve_batch, iters, fd, 0.0))
    assert ran == {}, ran
    for it in iters:
        it.close()


# ------------------------------------------------------------------------------------------------ 7. model route
def test_model_routes_with_fp_lockstep(dev):
    """``solve_shard_batched`` over the six dirichlet meshes with solver = anderson: the same u and nsteps with fp_lockstep True and
    False (the shard is below the vector-width switch: both routes run the 4-float kernels on the same block shapes), and with the
    key the launch record of item 4.  ``ModelDEQDSS.forward(list_of_batches)`` on two replicas: the same losses either way."""
    slv, batch = pkg("utilities.solver"), pkg("batch")
    S = _shard(False)
    T = 14

    def model(cls, **kw):
        net = getattr(pkg("model_psignn"), cls)(dict(latent_dim=10, n_layers=1, solver=slv.anderson, **kw))
        net.load_state_dict(S["sd"])
        return net.to(dev)

    runs = {}
    for key in (False, True):
        net = model("ModelPSIGNN", fw_tol=0.0, fw_thres=T, fp_lockstep=key).eval()
        runs[key], ran = _profiled(lambda: batch.solve_shard_batched(net, S["meshes"], dev))
        if key:
            for name in FP_KERNELS:
                assert ran.get(name, (0,))[0] == T - 2, (name, ran.get(name))
            assert ran.get("k_f_tile", (0,))[0] == T, ran.get("k_f_tile")
        else:
            assert ran["k_and_check"][0] == len(S["meshes"]) * (T - 2)
    for (i, u, loss), (j, v, loss2) in zip(runs[False], runs[True]):
        assert i == j and torch.equal(u, v) and loss["nsteps"] == loss2["nsteps"], i
        assert float(loss["residual_loss"]) == float(loss2["residual_loss"]), i
    losses, checks, nsteps = {}, {}, {}
    for key in (False, True):
        net = model("ModelDEQDSS", fw_tol=0.0, fw_thres=T, fp_lockstep=key).train()
        torch.manual_seed(3)                                              # (the probes of the Jacobian regulariser)
        (_, losses[key]), ran = _profiled(lambda: net([S["mds"][1], S["mds"][3]]))
        checks[key] = ran["k_and_check"][0]
        nsteps[key] = [o["nstep"] for o in net.deqdss.last_forward]
    assert checks == {False: 2 * (T - 2), True: T - 2} and nsteps[False] == nsteps[True], (checks, nsteps)
    for k in losses[False]:
        assert losses[False][k].shape == (2,) and torch.equal(losses[False][k], losses[True][k]), k
