"""GPU: the batched adjoint solve (psignn_broyden_solve_adjoint_lin_batch) and the replica training route built on it
(DeepEquilibrium.train_forward_replicas, ModelDEQDSS.forward on a list, DataParallel(..., replicas=R)).

Bit-identity per mesh against psignn_broyden_solve_adjoint_lin on the same solver objects; the adjoint equation against the CPU
oracle; refusals decided on the host; one training step of three replicas against the stored float64 gradients.

Gate of the replica step.  The project's single-run bound is 1e-2 per replica and tensor (test_gpu_training._cmp: error over
den_r(k) = max(|want_r[k]|, 1e-4 scale_r), scale_r the largest tensor norm of replica r's truth).  The parameter gradient of a
replica step is the mean of the replicas' gradients, so by the triangle inequality
    |got[k] - mean_r want_r[k]| <= mean_r |got_r[k] - want_r[k]| <= 1e-2 * mean_r den_r(k)
which assumes nothing about cancellation between replicas.  The denominators come from the stored truths only."""
import os

import numpy as np
import pytest
import torch

from conftest import CASES, load_case, load_weights, pkg, rel_l2
from oracle import psignn_oracle as orc
from test_gpu_training import _fp64_training_step, _model

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
FIELDS = ("n_iter", "nstep", "stop_reason", "prot_break", "lowest", "rel_trace", "abs_trace")


def _shard(dev, mixed):
    """Meshes of the forward batched solver's ragged shards, their maps, H* from the forward batched solve at 1e-5 / 300, one
    seeded Gaussian grad per mesh, one linearisation per mesh built at its H*, adjoint solvers sized for the shard."""
    data, eng = pkg("data"), pkg("engine")
    sizes = (9, 40, 13, 58, 26) if mixed else (10, 13, 11, 26, 12, 40)
    sd = load_weights("mixed" if mixed else "dirichlet")
    net = (pkg("mixed") if mixed else pkg("model_psignn")).ModelPSIGNN(dict(latent_dim=10, n_layers=1, fw_tol=1e-5, fw_thres=300))
    net.load_state_dict(sd)
    net = net.to(dev).eval()
    meshes = [data.make_hex_problem(n, seed=s, mixed=mixed) for s, n in enumerate(sizes)]
    mds = [m.to(dev) for m in meshes]
    with torch.no_grad():
        fmaps = [net.deqdss.f.bind(net.autoencoder.encoder(md.x), md) for md in mds]
    assert all(f.plan.tiled and bool(f.plan.mixed) == mixed for f in fmaps)
    total = sum(f.plan.N for f in fmaps) * 10
    fw = [eng.DeviceBroyden(plan=f.plan, threshold=300, keep_trace=False, shard_elems=total) for f in fmaps]
    H = [o["result"] for o in eng.broyden_solve_batch(fw, fmaps, 1e-5)]
    for sv in fw:
        sv.close()
    grads = [torch.randn(h.shape, generator=torch.Generator().manual_seed(100 + i)).to(dev) for i, h in enumerate(H)]
    lins = [f.linearize_p(f.to_plan(h), neumann="stored" if mixed else None) for f, h in zip(fmaps, H)]
    solvers = [eng.DeviceBroyden(plan=f.plan, threshold=300, keep_trace=False, shard_elems=total) for f in fmaps]
    return dict(sd=sd, meshes=meshes, fmaps=fmaps, H=H, grads=grads, lins=lins, solvers=solvers, total=total)


def _close(S):
    for o in S["lins"] + S["solvers"]:
        o.close()


def _same(a, b):
    for k in FIELDS:
        assert a[k] == b[k], (k, a[k] if not isinstance(a[k], list) else "trace", b["n_iter"])
    assert torch.equal(a["result"], b["result"])


@pytest.mark.parametrize("family", ["dirichlet", "mixed"])
def test_batched_adjoint_bit_identical_on_ragged_shard(family, dev):
    """Every mesh of a ragged shard: all fields and bits of the batched adjoint solve equal psignn_broyden_solve_adjoint_lin on the
    same solver object, for two poll intervals; the meshes stop at different iterations and one runs to the threshold.  Mixed:
    handles with stored Neumann rows."""
    eng, nat = pkg("engine"), pkg("_native")
    S = _shard(dev, family == "mixed")
    assert eng.adjoint_batchable(S["solvers"], S["lins"])
    single = [sv.solve_adjoint(f, h, g, 1e-6, lin=l) for sv, f, h, g, l in zip(S["solvers"], S["fmaps"], S["H"], S["grads"], S["lins"])]
    nat.prof_enable(True)
    nat.prof_collect()
    outs = eng.broyden_solve_adjoint_batch(S["solvers"], S["lins"], S["grads"], 1e-6)
    ran = nat.prof_collect()
    nat.prof_enable(False)
    print(f"{family}: n_iter single {[o['n_iter'] for o in single]} batched {[o['n_iter'] for o in outs]}; "
          f"lowest {['%.2e' % o['lowest'] for o in outs]}; stop_reason {[o['stop_reason'] for o in outs]}")
    assert "k_vjp_lin_batch" in ran and "k_vjp_lin" not in ran and "k_vjp_lin_mixed" not in ran, sorted(ran)
    # one product, one x_next and one residual launch per lockstep iteration
    its = max(o["n_iter"] for o in outs)
    assert ran["k_vjp_lin_batch"][0] == ran["k_xnext"][0] == ran["k_addv_resid"][0] >= its
    for a, b in zip(single, outs):
        _same(a, b)
    outs3 = eng.broyden_solve_adjoint_batch(S["solvers"], S["lins"], S["grads"], 1e-6, poll_every=3)
    for a, b in zip(single, outs3):
        _same(a, b)
    assert len({o["n_iter"] for o in outs}) >= 3          # the meshes really stop at different iterations ...
    assert max(o["n_iter"] for o in outs) == 300          # ... and a mesh that has stopped is skipped while another runs on
    _close(S)


def test_batched_adjoint_run_to_run(dev):
    eng = pkg("engine")
    S = _shard(dev, False)
    a = eng.broyden_solve_adjoint_batch(S["solvers"], S["lins"], S["grads"], 1e-6)
    b = eng.broyden_solve_adjoint_batch(S["solvers"], S["lins"], S["grads"], 1e-6)
    for x, y in zip(a, b):
        _same(x, y)
    _close(S)


@pytest.mark.parametrize("family,picks", [("dirichlet", (0, 1)), ("mixed", (0,))])
def test_batched_adjoint_against_oracle(family, picks, dev):
    """The gates of test_adjoint_solve_through_linearisation on meshes of the batched solve: residual of the adjoint equation with
    the oracle's VJP below 1e-4 relative, and rel-L2 to the oracle's Broyden on the oracle's VJP below 1e-3 where both converged."""
    eng = pkg("engine")
    S = _shard(dev, family == "mixed")
    outs = eng.broyden_solve_adjoint_batch(S["solvers"], S["lins"], S["grads"], 1e-6)
    for i in picks:
        mesh, sd = S["meshes"][i], S["sd"]
        y, hs, gr = outs[i]["result"].cpu(), S["H"][i].cpu(), S["grads"][i].cpu()
        with torch.no_grad():
            h0 = orc.encoder(sd, mesh.x)
        r = orc.function_vjp(sd, hs, h0, mesh, y) + gr - y
        res = float(r.norm() / y.norm())
        want = orc.broyden(lambda v: orc.function_vjp(sd, hs, h0, mesh, v) + gr, torch.zeros_like(gr), threshold=300, eps=1e-6)
        err = rel_l2(y, want["result"])
        print(f"{family} mesh {i}: device lowest {outs[i]['lowest']:.2e} after {outs[i]['n_iter']}, oracle lowest {want['lowest']:.2e}; "
              f"adjoint residual {res:.2e}, rel-L2 to the oracle's solve {err:.2e}")
        assert res < 1e-4
        if outs[i]["lowest"] < 1e-6 and want["lowest"] < 1e-6:
            assert err < 1e-3
    _close(S)


def test_batched_adjoint_refusals(dev):
    """Shards the lockstep does not take: adjoint_batchable is False and the batched call raises with nothing launched."""
    eng, nat = pkg("engine"), pkg("_native")
    D, M = _shard(dev, False), _shard(dev, True)
    f0, f1, mf = D["fmaps"][0], D["fmaps"][1], M["fmaps"][0]
    tot = D["total"]
    mk = lambda f, **kw: eng.DeviceBroyden(plan=f.plan, threshold=300, keep_trace=False, **{"shard_elems": tot, **kw})
    s0, s1, sm = D["solvers"][0], D["solvers"][1], mk(mf)
    l0, l1 = D["lins"][0], D["lins"][1]
    g0, g1, gm = D["grads"][0], D["grads"][1], M["grads"][0]
    bf = mk(f1, history_dtype=torch.bfloat16)
    unbuilt = eng.Linearization(f1)
    direct = mf.linearize_p(mf.to_plan(M["H"][0]), neumann="direct")
    assert not direct.neumann_stored
    big = mk(f1, shard_elems=400_000_000)      # sized for another shard: another vector width / split layout
    assert not eng.shard_batchable([s0, big])
    cases = {
        "both families": ([s0, sm], [l0, M["lins"][0]], [g0, gm]),
        "bf16 history": ([s0, bf], [l0, l1], [g0, g1]),
        "handle of another plan": ([s0, s1], [l1, l0], [g0, g1]),
        "unbuilt handle": ([s0, s1], [l0, unbuilt], [g0, g1]),
        "mixed handle, neumann direct": ([sm], [direct], [gm]),
        "different size classes": ([s0, big], [l0, l1], [g0, g1]),
    }
    assert eng.adjoint_batchable([s0, s1], [l0, l1]) and eng.adjoint_batchable([sm], [M["lins"][0]])
    nat.prof_enable(True)
    for what, (svs, lins, grads) in cases.items():
        assert not eng.adjoint_batchable(svs, lins), what
        nat.prof_collect()
        with pytest.raises(nat.NativeError):
            eng.broyden_solve_adjoint_batch(svs, lins, grads, 1e-6)
        assert nat.prof_collect() == {}, what
    nat.prof_enable(False)
    for o in (sm, bf, unbuilt, direct, big):
        o.close()
    _close(D)
    _close(M)


# ---- training step of three replicas ------------------------------------------------------------------------------------
def _draw(name, draw):
    g, mesh = load_case(name)
    m = mesh.clone() if hasattr(mesh, "clone") else mesh
    if draw > 0:   # exactly the perturbation of test_training_step_gradients
        gen = torch.Generator().manual_seed(2000 + draw)
        m.x = mesh.x * (1 + 1e-7 * torch.randn(mesh.x.shape, generator=gen))
    return m


def _gate(got, wants, what, ref=None, tol=1e-2):
    """max over tensors k of |got[k] - mean_r ref_r[k]| / mean_r den_r(k), den_r from the truths ``wants``; asserted <= tol."""
    ref = wants if ref is None else ref
    scales = [max(float(t.double().norm()) for t in w.values()) for w in wants]
    worst, name = 0.0, None
    for k in wants[0]:
        mean = sum(r[k].detach().cpu().double() for r in ref) / len(ref)
        den = sum(max(float(w[k].double().norm()), 1e-4 * s) for w, s in zip(wants, scales)) / len(wants)
        e = float((got[k].detach().cpu().double() - mean).norm()) / den
        if e > worst:
            worst, name = e, k
    print(f"ADJOINT_BATCH {what}: worst |got - mean| / mean den = {worst:.3e} ({name})")
    assert worst <= tol, (what, name, worst)
    return worst


def _replica_step(net, meshes, dev, jw=0.0):
    nat = pkg("_native")
    net.zero_grad()
    us, ld = net([m.to(dev) for m in meshes])
    assert all(v.shape == (len(meshes),) for v in ld.values())
    loss = (ld["residual_loss"] + jw * ld["jacobian_loss"] + ld["encoder_loss"] + ld["autoencoder_loss"]).mean()
    nat.prof_enable(True)
    nat.prof_collect()
    loss.backward()
    ran = nat.prof_collect()
    nat.prof_enable(False)
    got = {k: p.grad.clone() for k, p in net.named_parameters()}
    assert all(float(o["lowest"]) < 1e-7 for o in net.deqdss.last_backward), [o["lowest"] for o in net.deqdss.last_backward]
    assert len(net.deqdss.last_forward) == len(meshes) and len(net.deqdss.last_probes) == len(meshes)
    return got, ran, ld


REPLICAS = {"dirichlet": [("hex13_dirichlet_s0", 0), ("hex13_dirichlet_s0", 1), ("original_dirichlet_s0", 0)],
            "mixed": [("hex13_mixed_s1", 0), ("hex13_mixed_s1", 1), ("hex13_mixed_s1", 2)]}


@pytest.mark.parametrize("family", ["dirichlet", "mixed"])
def test_replica_training_step_gradients(family, dev, monkeypatch):
    """One training step over R = 3 replicas whose float64 gradients the project holds: the parameter gradient (mean of the
    replicas') against the mean of the truths under the bound derived in the module docstring; against the mean of three
    single-batch steps on the linearised route; with the Jacobian regulariser; through the sequential fallback."""
    eng = pkg("engine")
    reps = REPLICAS[family]
    sd = load_weights(family)
    T = np.load(os.path.join(GOLDEN, "grad_truth_fp64.npz"))
    meshes = [_draw(n, d) for n, d in reps]
    kw = dict(fw_tol=1e-7, fw_thres=600, bw_tol=1e-7, bw_thres=400)
    if family == "mixed":
        kw["lin_neumann"] = "stored"
    net = _model(sd, dev, **kw).train()
    got, ran, _ = _replica_step(net, meshes, dev)
    wants = [{k: torch.from_numpy(T[f"{n}/{d}/{k}"]) for k in got} for n, d in reps]
    # the adjoint solves of the step ran in lockstep on the batched product
    assert "k_vjp_lin_batch" in ran and "k_vjp_tile_a" not in ran and "k_vjp_lin" not in ran and "k_vjp_lin_mixed" not in ran, sorted(ran)
    _gate(got, wants, f"{family} lockstep vs fp64 truth")
    # the existing route: three single-batch steps, linearised backward
    singles = []
    for m in meshes:
        one = _model(sd, dev, bw_linearize=True, **kw).train()
        u, ld = one(m.to(dev))
        (ld["residual_loss"] + ld["encoder_loss"] + ld["autoencoder_loss"]).backward()
        assert one.deqdss.last_backward["lowest"] < 1e-7
        singles.append({k: p.grad.clone() for k, p in one.named_parameters()})
    _gate(got, wants, f"{family} lockstep vs mean of single-batch steps", ref=singles)
    # Jacobian regulariser at 50 x weight (test_training_step_with_jacobian_regulariser), truth per replica with its probe
    jw = 50.0
    gotj, _, ldj = _replica_step(net, meshes, dev, jw=jw)
    assert ldj["jacobian_loss"].requires_grad
    wj = [_fp64_training_step(sd, m, jac_weight=jw, probe=p.cpu())[2] for m, p in zip(meshes, net.deqdss.last_probes)]
    wj = [{k: w[k] for k in gotj} for w in wj]
    # the regulariser's share of the mean gradient is not negligible (else this gate would not see it)
    mean = lambda ws, k: sum(w[k].double() for w in ws) / len(ws)
    share = max(float((mean(wj, k) - mean(wants, k)).norm()) for k in gotj) / max(float(mean(wj, k).norm()) for k in gotj)
    print("regulariser share of the mean gradient", share)
    assert share > 0.05
    _gate(gotj, wj, f"{family} lockstep with regulariser vs fp64 truth")
    # sequential fallback of the adjoint solves, forced on the host
    monkeypatch.setattr(eng, "adjoint_batchable", lambda solvers, lins: False)
    gots, rans, _ = _replica_step(_model(sd, dev, **kw).train(), meshes, dev)
    assert "k_vjp_lin_batch" not in rans and ("k_vjp_lin_mixed" if family == "mixed" else "k_vjp_lin") in rans, sorted(rans)
    _gate(gots, wants, f"{family} sequential fallback vs fp64 truth")


def test_replica_route_falls_back_where_lockstep_does_not_apply(dev):
    """A bf16 pair history is not batched: the host-side decision sends the replicas through the single-mesh paths, one after
    the other, with replica semantics (per-replica solver dicts, stacked losses, finite gradients)."""
    sd = load_weights("dirichlet")
    meshes = [_draw("hex13_dirichlet_s0", 0), _draw("original_dirichlet_s0", 0)]
    net = _model(sd, dev, fw_tol=1e-5, fw_thres=300, bw_tol=1e-6, bw_thres=300, broyden_history_dtype=torch.bfloat16).train()
    fmaps = [net.deqdss.f.bind(net.autoencoder.encoder(m.to(dev).x).detach(), m.to(dev)) for m in meshes]
    assert not net.deqdss.lockstep_applies(fmaps)
    us, ld = net([m.to(dev) for m in meshes])
    assert ld["residual_loss"].shape == (2,)
    nat = pkg("_native")
    nat.prof_enable(True)
    nat.prof_collect()
    (ld["residual_loss"] + ld["encoder_loss"] + ld["autoencoder_loss"]).mean().backward()
    ran = nat.prof_collect()
    nat.prof_enable(False)
    assert "k_vjp_lin_batch" not in ran
    assert len(net.deqdss.last_backward) == 2 and all(o is not None for o in net.deqdss.last_backward)
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in net.parameters())
    # a single batch behaves as before
    u, ld1 = net(meshes[0].to(dev))
    assert ld1["residual_loss"].dim() == 0


def test_trainer_with_replicas(dev, tmp_path):
    """The reference's main.py shape with num_gpus = 2 on one GPU: DataListLoader + DataParallel(net, replicas=2), two steps,
    checkpoint round trip."""
    loader, TrainModel = pkg("loader"), pkg("training_class").TrainModel
    sd = load_weights("dirichlet")
    graphs = [load_case(n)[1] for n in ("hex13_dirichlet_s0", "original_dirichlet_s0", "original_dirichlet_s1", "hex13_dirichlet_s0")]
    net = _model(sd, dev, fw_tol=1e-5, fw_thres=300, bw_tol=1e-6, bw_thres=300)
    wrapped = loader.DataParallel(net, replicas=2).to(dev)
    cfg = dict(loader_train=loader.DataListLoader(graphs, batch_size=2), loader_val=loader.DataListLoader(graphs[:2], batch_size=2),
               model=wrapped, config_model=net.config, lr_deq=1e-5, lr_ae=1e-5, sched_step_deq=0.5, sched_step_ae=0.5,
               path_ckpt=str(tmp_path), min_loss_save=1e9, max_epochs=1, gradient_clip=1e-2, sup_weight=0.0, jac_weight=0.0)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    tr = TrainModel(cfg)
    tr.train_model()      # one epoch = two steps of two replicas each
    assert len(tr.hist_train["loss"]) == 1 and np.isfinite(tr.hist_train["loss"][0]) and np.isfinite(tr.hist_val["loss"][0])
    assert isinstance(net.deqdss.last_backward, list) and len(net.deqdss.last_backward) == 2
    assert any(not torch.equal(before[k], v) for k, v in net.state_dict().items())
    net2 = _model(sd, dev)
    tr2 = TrainModel(dict(cfg, model=loader.DataParallel(net2, replicas=2).to(dev)))
    tr2.load_model(str(tmp_path / "running_model.pt"))
    assert tr2.hist_train == tr.hist_train
    assert all(torch.equal(a.cpu(), b.cpu()) for a, b in zip(net2.state_dict().values(), net.state_dict().values()))
    us, ld = wrapped.eval()(graphs[:2])
    assert len(us) == 2 and us[0].shape == (graphs[0].num_nodes, 1) and us[0].is_cuda and ld["residual_loss"].shape == (2,)
