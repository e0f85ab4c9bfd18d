"""Derivatives of multi-layer dirichlet blocks (n_layers = L > 1) on the GPU against the CPU oracle's autograd in float64.

The chain rule the library runs (csrc/fgnn_layers.hip): JVP t_{k+1} = J_k t_k, VJP w_k = J_k^T w_{k+1}, with J_k the
single-layer Jacobian of layer k at its own input state h_k, LayerNorm on the last layer only.  The entry points take no
h_initial: the Dirichlet rows of h_1..h_{L-1} are h's own, so every state differentiated here has h_initial's Dirichlet rows
(as every state f returns, and every fixed point, has).

Weights: seeded random blocks (as tests/test_gpu_parity.py::test_multi_layer_dirichlet) and a "stacked checkpoint": the
trained dirichlet checkpoint's layer 0 copied into layers 1..L-1 unchanged.  The oracle's float64 Broyden solve of the
stacked 2-layer block on hex13_dirichlet_s0 reaches rel 1.0e-8 in 11 steps (threshold 600, eps 1e-7), so no rescaling of
the copied update MLP is needed.

Tolerances: the single-layer gates (JVP 1e-5, VJP 2e-5 rel-L2).  Measured on MI355X at L = 2, 3 on both fixtures and every
tile size: 2.5e-7 - 8.4e-7."""
import contextlib

import pytest
import torch

from conftest import load_case, load_weights, pkg, rel_l2
from oracle import psignn_oracle as orc

pytestmark = pytest.mark.gpu

_EXTRA = ("x", "edge_attr", "prb_data", "sol")


def _stacked(L):
    sd = load_weights("dirichlet")
    out = dict(sd)
    for k, t in sd.items():
        for mod in ("phi_to_list", "phi_from_list", "update_list"):
            if f".f.{mod}.0." in k:
                for l in range(1, L):
                    out[k.replace(f"{mod}.0.", f"{mod}.{l}.")] = t.clone()
    return out


def _random(L, seed=5):
    torch.manual_seed(seed)
    net = pkg("model_psignn").ModelPSIGNN(dict(latent_dim=10, n_layers=L))
    for p in net.parameters():
        if p.dim() == 1:
            torch.nn.init.normal_(p, std=0.1)
    return {k: v.detach().clone() for k, v in net.state_dict().items()}


def _weights(kind, L):
    return _stacked(L) if kind == "stacked" else _random(L)


def _mesh64(mesh):
    m = mesh.clone()
    for a in _EXTRA:
        if getattr(m, a, None) is not None:
            setattr(m, a, getattr(m, a).double())
    return m


def _sd64(sd):
    return {k: v.double() for k, v in sd.items()}


def _setup(mesh, sd, dev, tile_target=0, seed=11):
    """(fmap, h0, h): h random with h0's Dirichlet rows; h0 = the encoder of the mesh's input."""
    eng = pkg("engine")
    md = mesh.to(dev)
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        h0 = orc.encoder(sd, mesh.x).float()
    h = torch.randn(mesh.num_nodes, 10, generator=gen)
    idx = torch.where(mesh.tags == 1)[0]
    h[idx] = h0[idx]
    plan = eng.MeshPlan(md, tile_target=tile_target)
    fmap = eng.FixedPointMap(plan, eng.PackedWeights(sd, dev), h0.to(dev), md.prb_data)
    return fmap, h0, h


CASES = [("hex13_dirichlet_s0", 0), ("hex13_dirichlet_s0", -1), ("hex13_dirichlet_s0", 64), ("hex13_dirichlet_s0", 128),
         ("hex13_dirichlet_s0", 192), ("hex26_dirichlet_s0", 0), ("hex26_dirichlet_s0", -1)]


@pytest.mark.parametrize("kind", ["random", "stacked"])
@pytest.mark.parametrize("L", [2, 3])
@pytest.mark.parametrize("name,tt", CASES)
def test_jvp_vjp_against_oracle(name, tt, L, kind, dev):
    _, mesh = load_case(name)
    sd = _weights(kind, L)
    fmap, h0, h = _setup(mesh, sd, dev, tt)
    assert fmap.plan.tiled == (tt != -1)
    gen = torch.Generator().manual_seed(12)
    v, w = torch.randn(mesh.num_nodes, 10, generator=gen), torch.randn(mesh.num_nodes, 10, generator=gen)
    m64, s64 = _mesh64(mesh), _sd64(sd)
    jv_ref = orc.function_jvp(s64, h.double(), h0.double(), m64, v.double())
    vj_ref = orc.function_vjp(s64, h.double(), h0.double(), m64, w.double())
    H, V, Wv = h.to(dev), v.to(dev), w.to(dev)
    jv, vj = fmap.jvp(H, V), fmap.vjp(H, Wv)
    e_jv, e_vj = rel_l2(jv, jv_ref), rel_l2(vj, vj_ref)
    print(f"ML_ERR {name} tt={tt} L={L} {kind}: jvp {e_jv:.2e} vjp {e_vj:.2e}")
    assert e_jv <= 1e-5, e_jv
    assert e_vj <= 2e-5, e_vj
    # plan-order forms: the same kernels on permuted rows -> the same bits
    Hp = fmap.to_plan(H)
    assert torch.equal(fmap.from_plan(fmap.vjp_p(Hp, fmap.to_plan(Wv))), vj)
    if fmap.plan.tiled:
        assert torch.equal(fmap.from_plan(fmap.jvp_p(Hp, fmap.to_plan(V))), jv)
    # reproducible: a second call gives the same bits (no atomics anywhere in the chain)
    assert torch.equal(fmap.jvp(H, V), jv) and torch.equal(fmap.vjp(H, Wv), vj)


@pytest.mark.parametrize("L", [2, 3])
def test_mixed_multi_layer_unchanged_route(L, dev):
    """A mixed block differentiates its last layer only: its layer workspace is one weight view, its JVP and VJP match the oracle."""
    eng, nat = pkg("engine"), pkg("_native")
    torch.manual_seed(6)
    net = pkg("mixed").ModelPSIGNN(dict(latent_dim=10, n_layers=L))
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    _, mesh = load_case("hex13_mixed_s1")
    md = mesh.to(dev)
    plan = eng.MeshPlan(md)
    assert int(nat.lib().psignn_f_layers_workspace_floats(plan.handle, L)) == 4096
    gen = torch.Generator().manual_seed(4)
    h0, h, w = (torch.randn(mesh.num_nodes, 10, generator=gen) for _ in range(3))
    fmap = eng.FixedPointMap(plan, eng.PackedWeights(sd, dev), h0.to(dev), md.prb_data, md.unit_normal_vector)
    want = orc.function_vjp(_sd64(sd), h.double(), h0.double(), _mesh64(mesh), w.double())
    assert rel_l2(fmap.vjp(h.to(dev), w.to(dev)), want) <= 2e-5
    want = orc.function_jvp(_sd64(sd), h.double(), h0.double(), _mesh64(mesh), w.double())
    assert rel_l2(fmap.jvp(h.to(dev), w.to(dev)), want) <= 1e-5


def test_layer_workspace_query(dev):
    eng, nat = pkg("engine"), pkg("_native")
    _, mesh = load_case("hex13_dirichlet_s0")
    for tt in (0, -1):
        plan = eng.MeshPlan(mesh.to(dev), tile_target=tt)
        q = lambda L: int(nat.lib().psignn_f_layers_workspace_floats(plan.handle, L))
        assert q(1) == 0
        assert [q(L) for L in (2, 3, 5)] == [(4 * L + 1) * mesh.num_nodes * 10 + 4096 for L in (2, 3, 5)]
        assert q(0) < 0 and q(65) < 0


@pytest.mark.parametrize("n,L", [(13, 2), (13, 3), (182, 2)])
def test_transpose_identity(n, L, dev):
    """<w, J v> = <J^T w, v> to fp32 summation error, also at ~100k nodes (make_hex_problem(182): 99 919 nodes)."""
    data = pkg("data")
    mesh = data.make_hex_problem(n, seed=0, compute_sol=False)
    sd = _random(L, seed=8)
    for tt in (0, -1):
        fmap, _, h = _setup(mesh, sd, dev, tt, seed=13)
        gen = torch.Generator().manual_seed(14)
        v, w = torch.randn(mesh.num_nodes, 10, generator=gen).to(dev), torch.randn(mesh.num_nodes, 10, generator=gen).to(dev)
        H = h.to(dev)
        jv, vj = fmap.jvp(H, v).double(), fmap.vjp(H, w).double()
        lhs, rhs = float((w.double() * jv).sum()), float((vj * v.double()).sum())
        r = abs(lhs - rhs) / (float(w.double().norm()) * float(jv.norm()))
        print(f"ML_ADJ n={n} L={L} tt={tt}: {r:.2e}")
        assert r <= 1e-6, r


@contextlib.contextmanager
def _float64():
    """The oracle's Broyden allocates its low-rank factors in the default dtype."""
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        yield
    finally:
        torch.set_default_dtype(old)


def _oracle_fixed_point(sd, mesh, h0):
    s64, m64 = _sd64(sd), _mesh64(mesh)
    h0d = h0.double()
    with _float64():
        out = orc.broyden(lambda H: orc.function_forward(s64, H, h0d, m64), h0d, threshold=600, eps=1e-10)
    return out["result"]


@pytest.mark.parametrize("tt", [0, -1])
def test_adjoint_solve_two_layers(tt, dev):
    """implicit_backward's device Broyden adjoint solve at L = 2 against the float64 oracle's solution of y = J^T y + g at the
    oracle's fixed point; the layer state is evaluated once per solve, not per iteration."""
    nat, eng = pkg("_native"), pkg("engine")
    _, mesh = load_case("hex13_dirichlet_s0")
    sd = _stacked(2)
    fmap, h0, _ = _setup(mesh, sd, dev, tt)
    hs64 = _oracle_fixed_point(sd, mesh, h0)
    gen = torch.Generator().manual_seed(21)
    grad = torch.randn(mesh.num_nodes, 10, generator=gen)
    s64, m64 = _sd64(sd), _mesh64(mesh)
    g64 = grad.double()
    with _float64():
        ref = orc.broyden(lambda y: orc.function_vjp(s64, hs64, h0.double(), m64, y) + g64, torch.zeros_like(g64),
                          threshold=600, eps=1e-12)["result"]
    sv = eng.DeviceBroyden(plan=fmap.plan, threshold=200, keep_trace=False)
    try:
        nat.prof_enable(True)
        nat.prof_collect()
        try:
            out = sv.solve_adjoint(fmap, hs64.float().to(dev), grad.to(dev), 1e-9)
            ran = nat.prof_collect()
        finally:
            nat.prof_enable(False)
    finally:
        sv.close()
    e = rel_l2(out["result"], ref)
    print(f"ML_ADJSOLVE tt={tt}: {e:.2e} nstep {out['nstep']} launches {ran}")
    assert e <= 2e-5, e
    states = "k_f_tile_layer" if fmap.plan.tiled else "k_node"
    last = "k_vjp_tile_a" if fmap.plan.tiled else "k_vjp_local"
    first = "k_vjp_tile_a_noln" if fmap.plan.tiled else "k_vjp_local_noln"
    n_products = ran[last][0]
    assert n_products > 2 and ran[first][0] == n_products
    assert ran[states][0] == 1, ran[states]     # h_1 at h*, once per solve
    # the model's route: implicit_backward with the Broyden adjoint solve
    model = pkg("model_psignn").ModelPSIGNN(dict(latent_dim=10, n_layers=2, bw_tol=1e-9, bw_thres=200)).to(dev)
    model.load_state_dict(sd)
    md = mesh.to(dev)
    eng.plan_for(md)
    md._psignn_plan = (md._psignn_plan[0], fmap.plan)   # the cached plan of this batch: the one under test
    got = model.deqdss.implicit_backward(hs64.float().to(dev), h0.to(dev), md, grad.to(dev))
    assert rel_l2(got["result"], ref) <= 2e-5


def test_newton_krylov_and_power_method_two_layers(dev):
    """newton_krylov (the plan-order JVP chain) reaches the oracle's fixed point of the stacked 2-layer block from five
    Broyden steps; the power method (VJP chain) runs and is bitwise reproducible."""
    slv = pkg("utilities.solver")
    _, mesh = load_case("hex13_dirichlet_s0")
    sd = _stacked(2)
    fmap, h0, _ = _setup(mesh, sd, dev)
    hs64 = _oracle_fixed_point(sd, mesh, h0)
    warm = slv.broyden(fmap, h0.to(dev), threshold=5, eps=1e-12)
    out = slv.newton_krylov(fmap, h0.to(dev), threshold=40, eps=2e-7, inner_m=80, warm_start=5)
    e = rel_l2(out["result"], hs64)
    print(f"ML_NK: {e:.2e} lowest {out['lowest']:.2e} after 5 Broyden steps {warm['lowest']:.2e} nstep {out['nstep']}")
    assert warm["lowest"] > 1e3 * out["lowest"]   # the Newton steps, not the warm start, reach the fixed point
    assert out["lowest"] < 1e-6 and e <= 1e-5, (e, out["lowest"])
    model = pkg("model_psignn").ModelPSIGNN(dict(latent_dim=10, n_layers=2)).to(dev)
    model.load_state_dict(sd)
    md = mesh.to(dev)
    v0 = torch.randn(mesh.num_nodes, 10, generator=torch.Generator().manual_seed(3)).to(dev)
    hs = hs64.float().to(dev)
    a = model.deqdss.power_method(hs, h0.to(dev), md, n_iters=20, v0=v0)
    b = model.deqdss.power_method(hs, h0.to(dev), md, n_iters=20, v0=v0)
    assert torch.equal(a[0], b[0]) and float(a[1]) == float(b[1])
    assert torch.isfinite(a[0]).all() and float(a[1]) > 0.0


def test_dirichlet_rows_of_the_state_stand_for_h_initial(dev):
    """The documented rule of the derivative entry points, which take no h_initial: at a state whose Dirichlet rows differ
    from h_initial's, the multi-layer VJP / JVP are those of the block whose h_initial has h's Dirichlet rows."""
    _, mesh = load_case("hex13_dirichlet_s0")
    sd = _random(2)
    fmap, h0, _ = _setup(mesh, sd, dev)
    gen = torch.Generator().manual_seed(31)
    h, w = torch.randn(mesh.num_nodes, 10, generator=gen), torch.randn(mesh.num_nodes, 10, generator=gen)
    idx = torch.where(mesh.tags == 1)[0]
    assert not torch.equal(h[idx], h0[idx])
    h0_as_h = h0.clone()
    h0_as_h[idx] = h[idx]
    m64, s64 = _mesh64(mesh), _sd64(sd)
    assert rel_l2(fmap.vjp(h.to(dev), w.to(dev)), orc.function_vjp(s64, h.double(), h0_as_h.double(), m64, w.double())) <= 2e-5
    assert rel_l2(fmap.jvp(h.to(dev), w.to(dev)), orc.function_jvp(s64, h.double(), h0_as_h.double(), m64, w.double())) <= 1e-5


def _errs(got, want, floor_scale):
    return {k: float((got[k].detach().cpu().double() - w.double()).norm()) / max(float(w.double().norm()), 1e-4 * floor_scale)
            for k, w in want.items()}


def _cmp(got, want, tol, floor_scale, fp32=None):
    """max over tensors of ||got - want|| / max(||want||, 1e-4 * floor_scale) against tol -- or, per tensor, against twice the
    error of the oracle's own float32 evaluation (fp32: its gradients) where that is larger.  The shared alpha of a stacked
    checkpoint is such a tensor: its gradient (|g| ~ 2e-5 of the largest) is a sum over the layers that cancels, and float32
    autograd misses it by 2.7e-4 (L = 2) / 5.6e-4 (L = 3) in this measure."""
    errs = _errs(got, want, floor_scale)
    bound = {k: tol for k in want}
    if fp32 is not None:
        e32 = _errs(fp32, want, floor_scale)
        bound = {k: max(tol, 2.0 * e32[k]) for k in want}
    bad = {k: (round(e, 7), round(bound[k], 7)) for k, e in errs.items() if e >= bound[k]}
    assert not bad, bad
    return max(errs.values())


def _zeros_for_unused(g, sd):
    return {k: (torch.zeros_like(sd["deqdss.f." + k]).double() if t is None else t) for k, t in g.items()}


@pytest.mark.parametrize("kind", ["random", "stacked"])
@pytest.mark.parametrize("tt", [0, -1])
@pytest.mark.parametrize("L", [2, 3])
def test_param_vjp_against_oracle(L, tt, kind, dev):
    """Every named gradient (incl. *_list.1.*, the shared alpha and laynorm), w^T df/dh and w^T df/dh_init against the
    float64 oracle's autograd; the plan-order entry point gives the same bits on tiled plans."""
    _, mesh = load_case("hex13_dirichlet_s0")
    sd = _weights(kind, L)
    fmap, h0, h = _setup(mesh, sd, dev, tt)
    w = torch.randn(mesh.num_nodes, 10, generator=torch.Generator().manual_seed(17))
    want, want_h, want_init = orc.function_param_vjp(_sd64(sd), h.double(), h0.double(), _mesh64(mesh), w.double())
    grads, dh, dinit = fmap.param_vjp_init(h.to(dev), w.to(dev))
    assert set(grads) == set(want) and any("_list.2." in k for k in grads) == (L == 3)
    want32, _, _ = orc.function_param_vjp(sd, h, h0, mesh, w)
    scale = max(float(t.norm()) for t in want.values())
    e = _cmp(grads, want, 1e-4, scale, want32)
    e_h, e_init = rel_l2(dh, want_h), rel_l2(dinit, want_init)
    print(f"ML_PGRAD L={L} tt={tt} {kind}: params {e:.2e} dh {e_h:.2e} dh_init {e_init:.2e}")
    assert e_h <= 2e-5 and e_init <= 2e-5
    if fmap.plan.tiled:
        eng = pkg("engine")
        flat, out_p = fmap.param_vjp_p(fmap.to_plan(h.to(dev)), fmap.to_plan(w.to(dev)))
        named = eng.unpack_param_grads(flat, L, False)
        assert all(torch.equal(named[k], grads[k]) for k in grads)
        assert torch.equal(fmap.from_plan(out_p), dh)
    again = fmap.param_vjp_init(h.to(dev), w.to(dev))
    assert all(torch.equal(again[0][k], grads[k]) for k in grads) and torch.equal(again[2], dinit)


@pytest.mark.parametrize("tt", [0, -1])
def test_mixed_two_layer_param_vjp_and_vjp_backward(tt, dev):
    """Mixed block, L = 2: the last layer's gradients (and phi_neumann / update_neumann, alpha, laynorm) equal the oracle's,
    layer 0's are exactly zero; likewise for the backward of the VJP."""
    eng = pkg("engine")
    torch.manual_seed(6)
    net = pkg("mixed").ModelPSIGNN(dict(latent_dim=10, n_layers=2))
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    _, mesh = load_case("hex13_mixed_s1")
    md = mesh.to(dev)
    fmap = None
    gen = torch.Generator().manual_seed(4)
    h0, h, w, gb = (torch.randn(mesh.num_nodes, 10, generator=gen) for _ in range(4))
    fmap = eng.FixedPointMap(eng.MeshPlan(md, tile_target=tt), eng.PackedWeights(sd, dev), h0.to(dev), md.prb_data,
                             md.unit_normal_vector)
    s64, m64 = _sd64(sd), _mesh64(mesh)
    want, want_h, want_init = orc.function_param_vjp(s64, h.double(), h0.double(), m64, w.double())
    want = _zeros_for_unused(want, sd)   # autograd leaves no gradient on the layers that do not act
    grads, dh, dinit = fmap.param_vjp_init(h.to(dev), w.to(dev))
    zero = [k for k in grads if "_list.0." in k]
    assert zero and all(float(grads[k].abs().max()) == 0.0 for k in zero)
    scale = max(float(t.norm()) for t in want.values())
    _cmp(grads, want, 1e-4, scale)
    assert rel_l2(dh, want_h) <= 2e-5 and rel_l2(dinit, want_init) <= 2e-5
    bw, bh, _ = orc.function_vjp_backward(s64, h.double(), h0.double(), m64, w.double(), gb.double())
    g2, d2 = fmap.vjp_backward(h.to(dev), w.to(dev), gb.to(dev))
    assert all(float(g2[k].abs().max()) == 0.0 for k in zero)
    scale = max(float(t.norm()) for t in bw.values())
    e = _cmp(g2, bw, 1e-4, scale)
    print(f"ML_MIXED tt={tt}: vjp_backward params {e:.2e} dh {rel_l2(d2, bh):.2e}")
    assert rel_l2(d2, bh) <= 1e-4


@pytest.mark.parametrize("kind", ["random", "stacked"])
@pytest.mark.parametrize("tt", [0, -1])
def test_vjp_backward_two_layers(tt, kind, dev):
    """Backward of the VJP (the Jacobian regulariser's double backward) at L = 2 against the float64 oracle."""
    _, mesh = load_case("hex13_dirichlet_s0")
    sd = _weights(kind, 2)
    fmap, h0, h = _setup(mesh, sd, dev, tt)
    gen = torch.Generator().manual_seed(19)
    v, gb = torch.randn(mesh.num_nodes, 10, generator=gen), torch.randn(mesh.num_nodes, 10, generator=gen)
    want, want_h, _ = orc.function_vjp_backward(_sd64(sd), h.double(), h0.double(), _mesh64(mesh), v.double(), gb.double())
    want32, _, _ = orc.function_vjp_backward(sd, h, h0, mesh, v, gb)
    grads, dh = fmap.vjp_backward(h.to(dev), v.to(dev), gb.to(dev))
    scale = max(float(t.norm()) for t in want.values())
    e = _cmp(grads, want, 1e-4, scale, want32)
    print(f"ML_JR tt={tt} {kind}: params {e:.2e} dh {rel_l2(dh, want_h):.2e}")
    assert rel_l2(dh, want_h) <= 1e-4
    g2, d2 = fmap.vjp_backward(h.to(dev), v.to(dev), gb.to(dev))
    assert all(torch.equal(g2[k], grads[k]) for k in grads) and torch.equal(d2, dh)


def _fp64_training_step(sd, mesh, **kw):
    sd64, m64 = _sd64(sd), _mesh64(mesh)
    if kw.get("probe") is not None:
        kw["probe"] = kw["probe"].double()
    with _float64():
        return orc.training_step(sd64, m64, fw_tol=1e-12, fw_thres=1500, bw_tol=1e-12, bw_thres=1500, **kw)


def _model2(sd, dev, **kw):
    cfg = dict(latent_dim=10, n_layers=2, solver=pkg("utilities.solver").broyden, fw_tol=1e-7, fw_thres=600, bw_tol=1e-7,
               bw_thres=400)
    cfg.update(kw)
    mixed = any(k.startswith("deqdss.f.phi_neumann") for k in sd)
    net = (pkg("mixed") if mixed else pkg("model_psignn")).ModelDEQDSS(cfg)
    net.load_state_dict(sd)
    return net.to(dev)


@pytest.mark.parametrize("jw", [0.0, 50.0])
def test_training_step_two_layers(jw, dev):
    """model.train(); loss.backward() with n_layers = 2 (stacked checkpoint) against the float64 truth of the oracle's
    training step, without and with the Jacobian regulariser (weighted 50x so that its share is visible)."""
    _, mesh = load_case("hex13_dirichlet_s0")
    sd = _stacked(2)
    net = _model2(sd, dev).train()
    u, ld = net(mesh.to(dev))
    loss = ld["residual_loss"] + jw * ld["jacobian_loss"] + ld["encoder_loss"] + ld["autoencoder_loss"]
    loss.backward()
    probe = net.deqdss.last_probe.cpu() if jw else None
    wl, wld, wg64, _, _ = _fp64_training_step(sd, mesh, jac_weight=jw, probe=probe)
    got = {k: p.grad for k, p in net.named_parameters()}
    assert set(got) == set(wg64) and all(got[k] is not None for k in got)
    scale = max(float(t.norm()) for t in wg64.values())
    e = _cmp(got, wg64, 1e-2, scale)
    print(f"ML_TRAIN jw={jw}: loss {float(loss):.6e} vs {float(wl):.6e}, worst gradient {e:.2e}")
    assert abs(float(loss) - float(wl)) < 5e-3 * float(wl)
    if jw:   # the regulariser entered the loss and its value matches the truth's
        assert abs(float(ld["jacobian_loss"]) - float(wld["jacobian_loss"])) < 2e-3 * float(wld["jacobian_loss"])


@pytest.mark.parametrize("kind", ["dirichlet", "mixed"])
def test_trainer_two_layers(kind, dev, tmp_path):
    """TrainModel with n_layers = 2 for both families: a few epochs run (dirichlet: they lower the loss; mixed, whose first
    layer does not act: they leave it untouched -- zero gradients under Adam), the checkpoint reloads, and one epoch with the
    Jacobian regulariser (jac_weight 1) runs."""
    import os
    TrainModel = pkg("training_class").TrainModel
    if kind == "dirichlet":
        sd, names = _stacked(2), ("hex13_dirichlet_s0", "original_dirichlet_s0")
    else:
        base = load_weights("mixed")
        sd = dict(base)
        for k, t in base.items():
            for mod in ("phi_to_list", "phi_from_list", "update_list"):
                if f".f.{mod}.0." in k:
                    sd[k.replace(f"{mod}.0.", f"{mod}.1.")] = t.clone()
        names = ("hex13_mixed_s1",)
    meshes = [load_case(n)[1].to(dev) for n in names]
    net = _model2(sd, dev, fw_tol=1e-5, fw_thres=300, bw_tol=1e-6, bw_thres=300, path_logs=str(tmp_path))
    cfg = dict(loader_train=meshes, loader_val=meshes[:1], model=net, config_model=net.config, lr_deq=1e-4, lr_ae=1e-4,
               sched_step_deq=0.5, sched_step_ae=0.5, path_ckpt=str(tmp_path), min_loss_save=1e9, max_epochs=3,
               gradient_clip=1e-2, sup_weight=0.0, jac_weight=0.0)
    tr = TrainModel(cfg)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    tr.train_model()
    print(f"ML_TRAINER {kind}: {tr.hist_train['loss']}")
    assert all(torch.isfinite(torch.tensor(tr.hist_train["loss"])))
    after = net.state_dict()
    assert any(not torch.equal(before[k], after[k]) for k in after if "_list.1." in k)
    if kind == "dirichlet":
        assert tr.hist_train["loss"][-1] < tr.hist_train["loss"][0]
        assert any(not torch.equal(before[k], after[k]) for k in after if "_list.0." in k)
    else:
        assert all(torch.equal(before[k], after[k]) for k in after if "_list.0." in k)
    assert os.path.exists(tmp_path / "running_model.pt")
    tr2 = TrainModel(dict(cfg, model=_model2(sd, dev)))
    tr2.load_model(str(tmp_path / "running_model.pt"))
    assert all(torch.equal(a.cpu(), b.cpu()) for a, b in zip(tr2.model.state_dict().values(), net.state_dict().values()))
    tr3 = TrainModel(dict(cfg, jac_weight=1.0, max_epochs=1, path_ckpt=None))
    tr3.train_model()
    assert torch.isfinite(torch.tensor(tr3.hist_train["loss"])).all() and tr3.hist_train["jacobian_loss"][0] > 0
