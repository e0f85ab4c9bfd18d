"""The tile form of the backward of the VJP (csrc/fgnn_tile_jr.hip; ``vjp_backward(..., tiled=True)``, ``vjp_backward_p``, model
key ``jac_backward = "tiled"``) against ``orc.function_vjp_backward`` in float64, with the measures and gates the gather form
is held to: the fixture gate of test_gpu_training.py::test_vjp_backward_parity, the per-tile / per-tensor rule of
test_gpu_plan_limits.py at the structure limits (768 LDS rows, 255-slot walks, pass B's two staging parts), and the single-run
bound of test_training_step_with_jacobian_regulariser through the model.

Lines starting with JR_TILED report, without gating, the per-tensor distance between the two routes: two float32 results
with different summation orders differ by up to the sum of their errors; the float64 gates are the test."""
import pytest
import torch

import limit_graphs as lg
from conftest import CASES, load_case, load_weights, pkg, rel_l2
from oracle import psignn_oracle as orc
from test_gpu_multilayer import _stacked
from test_gpu_plan_limits import TAU as LIMIT_TAU
from test_gpu_plan_limits import Run
from test_gpu_training import _bind, _cmp, _fp64_training_step, _model, _to64, _worst

pytestmark = pytest.mark.gpu

FIXTURES = ["original_dirichlet_s0", "hex13_dirichlet_s0", "hex26_dirichlet_s0"]


def _inputs(g, fmap, dev):
    """h, v, gbar of test_vjp_backward_parity."""
    h = torch.from_numpy(g["f1"])
    v = torch.randn(h.shape, generator=torch.Generator().manual_seed(31))
    gq = fmap.vjp(h.to(dev), v.to(dev)).cpu()
    return h, v, 2.0 * gq / h.numel()


def _want64(sd, mesh, g, h, v, gbar):
    s64, m64 = _to64(sd, mesh)
    want, want_h, _ = orc.function_vjp_backward(s64, h.double(), torch.from_numpy(g["h0"]).double(), m64, v.double(), gbar.double())
    return want, want_h


def _fixture_gate(what, grads, out_h, want, want_h):
    """test_vjp_backward_parity's gate: per tensor <= 2e-4 of the largest tensor's norm, dh <= 2e-4."""
    assert set(grads) == set(want)
    scale = max(float(t.norm()) for t in want.values())
    e = _cmp(grads, want, 2e-4, scale)
    eh = rel_l2(out_h, want_h)
    print(f"JR_TILED {what}: worst tensor {e:.2e}, dh {eh:.2e} vs float64")
    assert eh < 2e-4


def _route_distance(what, a, b):
    scale = max(float(t.norm()) for t in b.values())
    d = {k: float((a[k] - b[k]).double().norm()) / max(float(b[k].double().norm()), 1e-4 * scale) for k in b}
    k = max(d, key=d.get)
    print(f"JR_TILED {what}: tiled vs gather route, per tensor " + ", ".join(f"{n.split('deqdss.f.')[-1]} {e:.1e}" for n, e in d.items())
          + f"; worst {k} {d[k]:.2e}")


@pytest.mark.parametrize("name", FIXTURES)
def test_tiled_vjp_backward_parity(name, dev):
    eng = pkg("engine")
    g, mesh, md, sd, fmap = _bind(name, dev)
    assert fmap.plan.tiled and fmap.can_tile_vjp_backward()
    h, v, gbar = _inputs(g, fmap, dev)
    H, V, G = h.to(dev), v.to(dev), gbar.to(dev)
    want, want_h = _want64(sd, mesh, g, h, v, gbar)
    grads, out_h = fmap.vjp_backward(H, V, G, tiled=True)
    _fixture_gate(name, grads, out_h, want, want_h)
    # fixed summation order, no atomics: the same bits again
    g2, o2 = fmap.vjp_backward(H, V, G, tiled=True)
    assert all(torch.equal(grads[k], g2[k]) for k in grads) and torch.equal(out_h, o2)
    # the keyword is the plan-order entry between two permutations
    flat, out_p = fmap.vjp_backward_p(fmap.to_plan(H), fmap.to_plan(V), fmap.to_plan(G))
    named = eng.unpack_param_grads(flat, 1, False)
    assert all(torch.equal(named[k], grads[k]) for k in grads) and torch.equal(fmap.from_plan(out_p), out_h)
    # the gather route on the same inputs (default keyword): reported, not gated
    gg, og = fmap.vjp_backward(H, V, G)
    _route_distance(name, grads, gg)
    print(f"JR_TILED {name}: tiled vs gather route, dh {rel_l2(out_h, og):.2e}")


@pytest.mark.parametrize("name", lg.CASE_NAMES)
def test_tiled_vjp_backward_at_the_plan_limits(name, dev):
    r = Run(name, False, dev)
    fm = r.fm
    H, W, G = r.dev_(r.h), r.dev_(r.wv), r.dev_(r.gb)
    if not r.plan.tiled:
        assert not fm.can_tile_vjp_backward()
        with pytest.raises(pkg("_native").NativeError):
            fm.vjp_backward(H, W, G, tiled=True)
        with pytest.raises(pkg("_native").NativeError):
            fm.vjp_backward_p(H, W, G)
        return
    assert fm.can_tile_vjp_backward()
    want, want_h, _ = orc.function_vjp_backward(r.s64, r.h.double(), r.h0.double(), r.m64, r.wv.double(), r.gb.double())
    want32, want32_h, _ = orc.function_vjp_backward(r.sd, r.h, r.h0, r.m, r.wv, r.gb)
    g2, d2 = fm.vjp_backward(H, W, G, tiled=True)
    assert set(g2) == set(want)
    r.check_params("vjp_backward tiled", g2, want, want32, LIMIT_TAU["jr"])
    r.check("vjp_backward tiled dh", d2, want_h, want32_h, LIMIT_TAU["jr_h"])
    g3, d3 = fm.vjp_backward(H, W, G, tiled=True)
    assert all(torch.equal(g2[k], g3[k]) for k in g2) and torch.equal(d2, d3)


@pytest.mark.parametrize("tt", [32, 100])
def test_tiled_vjp_backward_other_tile_sizes(tt, dev):
    """Tiles that fill neither the workgroup nor their last wave (the sizes test_param_vjp_other_tile_sizes uses)."""
    eng = pkg("engine")
    g, mesh, md, sd, fmap = _bind("hex26_dirichlet_s0", dev)
    h, v, gbar = _inputs(g, fmap, dev)
    want, want_h = _want64(sd, mesh, g, h, v, gbar)
    fm = eng.FixedPointMap(eng.MeshPlan(md, tile_target=tt), fmap.weights, fmap.h0, md.prb_data, None)
    assert fm.plan.tiled and fm.can_tile_vjp_backward() and fm.plan.n_tiles > fmap.plan.n_tiles
    grads, out_h = fm.vjp_backward(h.to(dev), v.to(dev), gbar.to(dev), tiled=True)
    _fixture_gate(f"hex26 tile_target={tt}", grads, out_h, want, want_h)


def _step(net, mesh, dev, jw=1.0):
    u, ld = net(mesh.to(dev))
    loss = ld["residual_loss"] + jw * ld["jacobian_loss"] + ld["encoder_loss"] + ld["autoencoder_loss"]
    loss.backward()
    return ld, loss


def test_refusals_take_the_gather_route(dev):
    """A mixed plan, a two-layer dirichlet block and an untiled plan have no tile form: the entry points say so, and a model
    with jac_backward="tiled" trains on them through the gather kernels."""
    eng, nat = pkg("engine"), pkg("_native")
    # mixed plan
    g, mesh, md, sd, fmap = _bind("hex13_mixed_s1", dev)
    h, v, gbar = _inputs(g, fmap, dev)
    assert fmap.plan.tiled and fmap.plan.mixed and not fmap.can_tile_vjp_backward()
    with pytest.raises(nat.NativeError):
        fmap.vjp_backward(h.to(dev), v.to(dev), gbar.to(dev), tiled=True)
    with pytest.raises(nat.NativeError):
        fmap.vjp_backward_p(h.to(dev), v.to(dev), gbar.to(dev))
    net = _model(sd, dev, jac_backward="tiled").train()
    _step(net, mesh, dev)
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in net.parameters())
    # two-layer dirichlet block
    g, mesh = load_case("hex13_dirichlet_s0")
    sd2 = _stacked(2)
    md = mesh.to(dev)
    fm2 = eng.FixedPointMap(eng.plan_for(md), eng.PackedWeights(sd2, dev), torch.from_numpy(g["h0"]).to(dev), md.prb_data, None)
    assert fm2.plan.tiled and fm2.weights.n_layers == 2 and not fm2.can_tile_vjp_backward()
    h = torch.from_numpy(g["f1"]).to(dev)
    with pytest.raises(nat.NativeError):
        fm2.vjp_backward(h, torch.ones_like(h), torch.ones_like(h), tiled=True)
    net = _model(sd2, dev, n_layers=2, jac_backward="tiled").train()
    _step(net, mesh, dev)
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in net.parameters())
    # untiled plan of a single-layer dirichlet block
    flat = eng.FixedPointMap(eng.MeshPlan(md, tile_target=-1), eng.PackedWeights(load_weights("dirichlet"), dev),
                             torch.from_numpy(g["h0"]).to(dev), md.prb_data, None)
    assert not flat.plan.tiled and not flat.can_tile_vjp_backward()
    with pytest.raises(nat.NativeError):
        flat.vjp_backward(h, torch.ones_like(h), torch.ones_like(h), tiled=True)


def test_training_step_with_jacobian_regulariser_tiled(dev):
    """The step of test_training_step_with_jacobian_regulariser on hex13_dirichlet_s0 (its 50 x weight, its fixed probe) with
    jac_backward="tiled": every gradient against the float64 step with that test's single-run bound, and the regulariser's
    backward really ran on the tile kernels."""
    nat = pkg("_native")
    name, jw = "hex13_dirichlet_s0", 50.0
    g, mesh = load_case(name)
    sd = load_weights(CASES[name])
    net = _model(sd, dev, fw_tol=1e-7, fw_thres=600, jac_backward="tiled").train()
    nat.prof_enable(True)
    nat.prof_collect()
    try:
        torch.manual_seed(1234)
        ld, loss = _step(net, mesh, dev, jw)
        ran = nat.prof_collect()
    finally:
        nat.prof_enable(False)
    assert "k_jr_tile_a" in ran and "k_jr_tile_b" in ran and "k_jr_node" not in ran, sorted(ran)
    probe = net.deqdss.last_probe.cpu()
    wl, wld, wg64, _, _ = _fp64_training_step(sd, mesh, jac_weight=jw, probe=probe)
    assert abs(float(ld["jacobian_loss"]) - float(wld["jacobian_loss"])) < 2e-3 * float(wld["jacobian_loss"])
    assert abs(float(loss) - float(wl)) < 5e-3 * float(wl)
    got = {k: p.grad for k, p in net.named_parameters()}
    scale = max(float(t.norm()) for t in wg64.values())
    e_hip = _cmp(got, wg64, 1e-2, scale)       # the single-run bound of test_training_step_with_jacobian_regulariser
    # the gather route on the same step and probe: reported
    ref = _model(sd, dev, fw_tol=1e-7, fw_thres=600).train()
    torch.manual_seed(1234)
    _step(ref, mesh, dev, jw)
    assert torch.equal(ref.deqdss.last_probe.cpu(), probe)
    e_ref, k_ref = _worst({k: p.grad for k, p in ref.named_parameters()}, wg64, scale)
    print(f"JR_TILED training step: worst gradient error vs fp64 truth, tiled {e_hip:.2e}; gather route {e_ref:.2e} ({k_ref})")
