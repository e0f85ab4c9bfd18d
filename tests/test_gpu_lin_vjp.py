"""GPU: the transposed product of the stored linearisation (Linearization.vjp_p, csrc/fgnn_tile_lin.hip k_vjp_lin), the adjoint
solve through it (psignn_broyden_solve_adjoint_lin) and the model's opt-in ``bw_linearize``."""

import pytest
import torch

from conftest import CASES, load_case, load_weights, pkg, rel_l2
from oracle import psignn_oracle as orc

pytestmark = pytest.mark.gpu

NAMES = ["original_dirichlet_s0", "hex13_dirichlet_s0", "hex26_dirichlet_s0", "hex13_mixed_s1"]


def bind(name, dev, tile_target=0):
    g, mesh = load_case(name)
    sd = load_weights(CASES[name])
    eng = pkg("engine")
    md = mesh.to(dev)
    w = eng.PackedWeights(sd, dev)
    h0 = torch.from_numpy(g["h0"]).to(dev)
    plan = eng.plan_for(md) if tile_target == 0 else eng.MeshPlan(md, tile_target=tile_target)
    fmap = eng.FixedPointMap(plan, w, h0, md.prb_data, getattr(md, "unit_normal_vector", None))
    return g, mesh, md, sd, fmap


def adjoint_gap(lin, Wp, Vp):
    """|<w, J v> - <J^T w, v>| / (|w| |J v|), accumulated in float64."""
    jv = lin.jvp_p(Vp).double()
    jtw = lin.vjp_p(Wp).double()
    lhs = float((Wp.double() * jv).sum())
    rhs = float((jtw * Vp.double()).sum())
    return abs(lhs - rhs) / (float(Wp.double().norm()) * float(jv.norm()))


@pytest.mark.parametrize("name", NAMES)
def test_lin_vjp_parity(name, dev):
    """lin.vjp_p against the tiled VJP at the same state, the float64 golden VJP and the oracle's autograd VJP."""
    g, mesh, md, sd, fmap = bind(name, dev)
    assert fmap.can_linearize()
    if "jv_point" in g:
        hp = torch.from_numpy(g["jv_point"]).float().to(dev)
        w = torch.from_numpy(g["jv_dir"]).float().to(dev)
        Hp, Wp = fmap.to_plan(hp), fmap.to_plan(w)
        lin = fmap.linearize_p(Hp)
        got = fmap.from_plan(lin.vjp_p(Wp))
        assert rel_l2(got, g["vjp64"]) < 1e-5, rel_l2(got, g["vjp64"])
        assert rel_l2(got, fmap.from_plan(fmap.vjp_p(Hp, Wp))) < 2e-6
        lin.close()
    hp = torch.from_numpy(g["f1"])
    w = torch.randn(hp.shape, generator=torch.Generator().manual_seed(5))
    Hp, Wp = fmap.to_plan(hp.to(dev)), fmap.to_plan(w.to(dev))
    lin = fmap.linearize_p(Hp)
    got = lin.vjp_p(Wp)
    assert rel_l2(got, fmap.vjp_p(Hp, Wp)) < 2e-6, rel_l2(got, fmap.vjp_p(Hp, Wp))
    want = orc.function_vjp(sd, hp, torch.from_numpy(g["h0"]), mesh, w)
    assert rel_l2(fmap.from_plan(got), want) < 2e-5
    lin.close()


@pytest.mark.parametrize("name", NAMES)
def test_lin_vjp_is_the_transpose_of_lin_jvp(name, dev):
    g, mesh, md, sd, fmap = bind(name, dev)
    lin = fmap.linearize_p(fmap.to_plan(torch.from_numpy(g["f1"]).to(dev)))
    gen = torch.Generator().manual_seed(11)
    for _ in range(4):
        Wp = torch.randn(mesh.num_nodes, 10, generator=gen).to(dev)
        Vp = torch.randn(mesh.num_nodes, 10, generator=gen).to(dev)
        gap = adjoint_gap(lin, Wp, Vp)
        assert gap <= 1e-6, gap
    lin.close()


def test_lin_vjp_transpose_at_100k_nodes(dev):
    data, eng = pkg("data"), pkg("engine")
    sd = load_weights("dirichlet")
    mesh = data.make_hex_problem(182, seed=0, compute_sol=False)
    md = mesh.to(dev)
    with torch.no_grad():
        h0 = orc.encoder(sd, mesh.x)
    fm = eng.FixedPointMap(eng.MeshPlan(md), eng.PackedWeights(sd, dev), h0.to(dev), md.prb_data)
    Hp = fm.fp(fm.fp(fm.to_plan(fm.h0)))
    lin = fm.linearize_p(Hp)
    gen = torch.Generator().manual_seed(3)
    for _ in range(3):
        Wp = torch.randn(mesh.num_nodes, 10, generator=gen).to(dev)
        Vp = torch.randn(mesh.num_nodes, 10, generator=gen).to(dev)
        gap = adjoint_gap(lin, Wp, Vp)
        assert gap <= 1e-6, gap
    assert rel_l2(lin.vjp_p(Wp), fm.vjp_p(Hp, Wp)) < 2e-6
    lin.close()


@pytest.mark.parametrize("name", ["hex13_dirichlet_s0", "hex13_mixed_s1"])
def test_lin_vjp_operator_properties(name, dev):
    nat = pkg("_native")
    eng = pkg("engine")
    g, mesh, md, sd, fmap = bind(name, dev)
    Hp = fmap.to_plan(torch.from_numpy(g["f1"]).to(dev))
    lin = eng.Linearization(fmap)
    gen = torch.Generator().manual_seed(2)
    Wp = torch.randn(mesh.num_nodes, 10, generator=gen).to(dev)
    with pytest.raises(nat.NativeError):
        lin.vjp_p(Wp)                       # before any build
    fmap.linearize_p(Hp, lin)
    with pytest.raises(nat.NativeError):
        lin.vjp_p(Wp, out=Wp)               # in place
    U = torch.roll(Wp, 5, 0).contiguous()
    comb = lin.vjp_p(1.5 * Wp - 0.25 * U)
    assert rel_l2(comb, 1.5 * lin.vjp_p(Wp) - 0.25 * lin.vjp_p(U)) < 2e-6
    a = lin.vjp_p(Wp)
    assert torch.equal(a, lin.vjp_p(Wp))
    out = torch.empty_like(Wp)
    assert lin.vjp_p(Wp, out=out) is out and torch.equal(out, a)
    # a rebuild at another state gives that state's VJP (the transposed masks are refreshed)
    H2 = fmap.fp(fmap.fp(Hp))
    assert fmap.linearize_p(H2, lin) is lin
    assert rel_l2(lin.vjp_p(Wp), fmap.vjp_p(H2, Wp)) < 2e-6
    assert not torch.equal(lin.vjp_p(Wp), a)
    lin.close()


@pytest.mark.parametrize("target", [64, 128, 192])
def test_lin_vjp_other_tile_sizes(target, dev):
    g, mesh, md, sd, fmap = bind("hex26_dirichlet_s0", dev, tile_target=target)
    assert fmap.plan.tiled
    Hp = fmap.to_plan(torch.from_numpy(g["f1"]).to(dev))
    lin = fmap.linearize_p(Hp)
    gen = torch.Generator().manual_seed(4)
    Wp = torch.randn(mesh.num_nodes, 10, generator=gen).to(dev)
    Vp = torch.randn(mesh.num_nodes, 10, generator=gen).to(dev)
    assert rel_l2(lin.vjp_p(Wp), fmap.vjp_p(Hp, Wp)) < 2e-6
    assert adjoint_gap(lin, Wp, Vp) <= 1e-6
    lin.close()


def test_lin_vjp_degenerate_graphs(dev):
    """The graphs of test_plan_degenerate_graphs (no edges, self loops only, isolated nodes and duplicate edges): the
    transposed product against the tiled VJP and the transpose identity."""
    eng, data = pkg("engine"), pkg("data")
    N = 5
    base = dict(x=torch.zeros(N, 1), y=torch.zeros(N, 1), sol=torch.zeros(N, 1), prb_data=torch.zeros(N, 2),
                tags=torch.tensor([[1.], [0.], [0.], [0.], [1.]]), pos=torch.zeros(N, 2))
    sd = load_weights("dirichlet")
    gen = torch.Generator().manual_seed(7)
    n_lin = 0
    for ei in (torch.zeros(2, 0, dtype=torch.long), torch.tensor([[0, 1, 2], [0, 1, 2]]),
               torch.tensor([[1, 1, 1, 3, 2], [2, 2, 3, 1, 2]]), torch.tensor([[0, 1, 2, 3, 4, 1], [1, 2, 3, 4, 3, 0]])):
        m = data.MeshData(edge_index=ei, edge_attr=torch.randn(ei.shape[1], 3, generator=gen),
                          a_ij=torch.randn(ei.shape[1], 1, generator=gen), **base)
        plan = eng.MeshPlan(m.to(dev))
        h0 = torch.randn(N, 10, generator=gen)
        fm = eng.FixedPointMap(plan, eng.PackedWeights(sd, dev), h0.to(dev), m.prb_data.to(dev))
        if not fm.can_linearize():
            continue
        n_lin += 1
        Hp = fm.to_plan(h0.to(dev))
        lin = fm.linearize_p(Hp)
        Wp = torch.randn(N, 10, generator=gen).to(dev)
        Vp = torch.randn(N, 10, generator=gen).to(dev)
        got = lin.vjp_p(Wp)
        want = fm.vjp_p(Hp, Wp)
        assert bool(torch.isfinite(got).all())
        assert rel_l2(got, want) < 2e-6 or float((got - want).abs().max()) == 0.0, ei.tolist()
        jv = lin.jvp_p(Vp).double()
        lhs, rhs = float((Wp.double() * jv).sum()), float((got.double() * Vp.double()).sum())
        assert abs(lhs - rhs) <= 1e-6 * float(Wp.double().norm()) * max(float(jv.norm()), 1e-30)
        lin.close()
    assert n_lin > 0


def test_lin_vjp_dirichlet_rows_carry_no_cotangent(dev):
    g, mesh, md, sd, fmap = bind("hex13_dirichlet_s0", dev)
    Hp = fmap.to_plan(torch.from_numpy(g["f1"]).to(dev))
    lin = fmap.linearize_p(Hp)
    dmask = (mesh.tags.reshape(mesh.num_nodes, -1)[:, 0] == 1).float().unsqueeze(1)
    assert 0 < float(dmask.sum()) < mesh.num_nodes
    w = torch.randn(mesh.num_nodes, 10, generator=torch.Generator().manual_seed(8)) * dmask
    got = lin.vjp_p(fmap.to_plan(w.to(dev)))
    assert float(got.abs().max()) == 0.0
    lin.close()


@pytest.mark.parametrize("name", ["hex13_dirichlet_s0", "hex13_mixed_s1"])
def test_adjoint_solve_through_linearisation(name, dev):
    g, mesh, md, sd, fmap = bind(name, dev)
    eng = pkg("engine")
    h_star = torch.from_numpy(g["broyden_e7_result"])
    h0 = torch.from_numpy(g["h0"])
    grad = torch.randn(h_star.shape, generator=torch.Generator().manual_seed(9))
    lin = fmap.linearize_p(fmap.to_plan(h_star.to(dev)))
    sv = eng.DeviceBroyden(fmap.plan, 600, keep_trace=False)
    out = sv.solve_adjoint(fmap, h_star.to(dev), grad.to(dev), 1e-6, lin=lin)
    assert out["lowest"] < 1e-6
    y = out["result"]
    r = orc.function_vjp(sd, h_star, h0, mesh, y.cpu()) + grad - y.cpu()
    assert float(r.norm() / y.cpu().norm()) < 1e-4
    base = sv.solve_adjoint(fmap, h_star.to(dev), grad.to(dev), 1e-6)
    assert rel_l2(y, base["result"]) < 1e-3
    # a linearisation of another plan is refused
    other = bind("hex26_dirichlet_s0", dev)[4]
    lin2 = other.linearize_p(other.to_plan(other.h0))
    with pytest.raises(pkg("_native").NativeError):
        sv.solve_adjoint(fmap, h_star.to(dev), grad.to(dev), 1e-6, lin=lin2)
    lin2.close()
    lin.close()


def _model(sd, dev, **kw):
    solver = pkg("utilities.solver")
    cfg = dict(latent_dim=10, n_layers=1, solver=solver.broyden, fw_tol=1e-7, fw_thres=600, bw_tol=1e-6, bw_thres=600)
    cfg.update(kw)
    mixed = any(k.startswith("deqdss.f.phi_neumann") for k in sd)
    net = (pkg("mixed") if mixed else pkg("model_psignn")).ModelDEQDSS(cfg)
    net.load_state_dict(sd)
    return net.to(dev)


@pytest.mark.parametrize("name", ["hex13_dirichlet_s0", "hex13_mixed_s1"])
def test_model_opt_in_backward_routes(name, dev):
    g, mesh, md, sd, fmap = bind(name, dev)
    solver = pkg("utilities.solver")
    h_star = torch.from_numpy(g["broyden_e7_result"]).to(dev)
    h0 = torch.from_numpy(g["h0"]).to(dev)
    grad = torch.randn(h_star.shape, generator=torch.Generator().manual_seed(9)).to(dev)
    ref, lin = _model(sd, dev), _model(sd, dev, bw_linearize=True)
    assert "bw_linearize" not in ref.deqdss.config_deq and lin.deqdss.config_deq["bw_linearize"] is True
    a = ref.deqdss.implicit_backward(h_star, h0, md, grad)
    b = lin.deqdss.implicit_backward(h_star, h0, md, grad)
    assert a["lowest"] < 1e-6 and b["lowest"] < 1e-6
    assert rel_l2(b["result"], a["result"]) < 1e-3
    assert getattr(lin.deqdss, "_bw_lin", None) is not None and getattr(ref.deqdss, "_bw_lin", None) is None
    # the generic solver(f, x0, ...) route
    lin.deqdss.config_deq["solver"] = lambda f, x0, threshold, eps: solver.broyden(f, x0, threshold=threshold, eps=eps)
    c = lin.deqdss.implicit_backward(h_star, h0, md, grad)
    lin.deqdss.config_deq["solver"] = solver.broyden
    assert rel_l2(c["result"], a["result"]) < 1e-3
    # diagnostics on fixed probes / start vector
    gen = torch.Generator().manual_seed(21)
    probes = [torch.randn(h_star.shape, generator=gen).to(dev) for _ in range(3)]
    ja = ref.deqdss.jac_loss_estimate(h_star, h0, md, probes=probes)
    jb = lin.deqdss.jac_loss_estimate(h_star, h0, md, probes=probes)
    jc = ref.deqdss.jac_loss_estimate(h_star, h0, md, probes=probes, linearize=True)
    assert abs(float(jb) - float(ja)) < 1e-5 * float(ja) and abs(float(jc) - float(ja)) < 1e-5 * float(ja)
    v0 = torch.randn(h_star.shape, generator=gen).to(dev)
    ea, ra = ref.deqdss.power_method(h_star, h0, md, n_iters=40, v0=v0)
    eb, rb = lin.deqdss.power_method(h_star, h0, md, n_iters=40, v0=v0)
    assert abs(float(rb) - float(ra)) < 2e-4 * float(ra)
    assert min(rel_l2(eb, ea), rel_l2(eb, -ea)) < 5e-3
    ec, rc = lin.deqdss.power_method(h_star, h0, md, n_iters=40, v0=v0, linearize=False)
    assert torch.equal(ec, ea) and float(rc) == float(ra)


@pytest.mark.parametrize("name", ["hex13_dirichlet_s0", "hex13_mixed_s1"])
def test_training_step_gradients_with_linearised_backward(name, dev):
    """One training step's parameter gradients with bw_linearize against the default path's (the bound of
    test_training_step_gradients: the fp32 gradient is a sample within 1e-2 of the truth; the two paths agree well inside it)."""
    g, mesh = load_case(name)
    sd = load_weights(CASES[name])
    grads = []
    for opt in (False, True):
        net = _model(sd, dev, fw_tol=1e-7, fw_thres=600, bw_tol=1e-7, bw_thres=400, bw_linearize=opt).train()
        torch.manual_seed(0)
        u, ld = net(mesh.to(dev))
        loss = ld["residual_loss"] + ld["encoder_loss"] + ld["autoencoder_loss"]
        loss.backward()
        assert net.deqdss.last_backward["lowest"] < 1e-7
        grads.append({k: p.grad.detach().double().cpu() for k, p in net.named_parameters()})
    scale = max(float(t.norm()) for t in grads[0].values())
    worst = max(float((grads[1][k] - w).norm()) / max(float(w.norm()), 1e-4 * scale) for k, w in grads[0].items())
    assert worst < 1e-2, worst


def test_fallback_where_no_linearisation(dev):
    """Untiled plan: bw_linearize silently takes today's path (bit-identical results).  Multi-layer dirichlet block: no
    linearisation is made, and the routes behave exactly as without the key."""
    g, mesh, md, sd, fmap = bind("hex13_dirichlet_s0", dev)
    eng, nat = pkg("engine"), pkg("_native")
    h_star = torch.from_numpy(g["broyden_e7_result"]).to(dev)
    h0 = torch.from_numpy(g["h0"]).to(dev)
    grad = torch.randn(h_star.shape, generator=torch.Generator().manual_seed(9)).to(dev)
    mu = mesh.to(dev)
    eng.plan_for(mu)
    mu._psignn_plan = (mu._psignn_plan[0], eng.MeshPlan(mu, tile_target=-1))   # the cached plan of this batch: untiled
    assert not eng.plan_for(mu).tiled
    ref, lin = _model(sd, dev), _model(sd, dev, bw_linearize=True)
    a = ref.deqdss.implicit_backward(h_star, h0, mu, grad)
    b = lin.deqdss.implicit_backward(h_star, h0, mu, grad)
    assert torch.equal(a["result"], b["result"])
    pa = ref.deqdss.power_method(h_star, h0, mu, n_iters=5, v0=grad)
    pb = lin.deqdss.power_method(h_star, h0, mu, n_iters=5, v0=grad)
    assert torch.equal(pa[0], pb[0]) and float(pa[1]) == float(pb[1])
    assert getattr(lin.deqdss, "_bw_lin", None) is None
    # multi-layer dirichlet block (random weights): nothing is linearised, the same outcome as the default route
    torch.manual_seed(0)
    cfg = dict(latent_dim=10, n_layers=2, fw_tol=1e-6, fw_thres=50, bw_tol=1e-6, bw_thres=50)
    m2 = pkg("model_psignn").ModelDEQDSS(cfg).to(dev)
    m2l = pkg("model_psignn").ModelDEQDSS(dict(cfg, bw_linearize=True)).to(dev)
    m2l.load_state_dict(m2.state_dict())
    fm2 = m2l.deqdss.f.bind(h0, md)
    assert not fm2.can_linearize() and m2l.deqdss._linearization(fm2, h_star) is None
    outs = []
    for net in (m2, m2l):
        try:
            outs.append(net.deqdss.power_method(h_star, h0, md, n_iters=3, v0=grad))
        except nat.NativeError as e:
            outs.append(type(e))
    if isinstance(outs[0], tuple):
        assert torch.equal(outs[0][0], outs[1][0])
    else:
        assert outs[0] is outs[1]


def _check_against_tiled_vjp(m, sd, dev, gen):
    eng = pkg("engine")
    plan = eng.MeshPlan(m.to(dev))
    N = m.num_nodes
    h0 = torch.randn(N, 10, generator=gen)
    fm = eng.FixedPointMap(plan, eng.PackedWeights(sd, dev), h0.to(dev), m.prb_data.to(dev))
    assert fm.can_linearize()
    Hp = fm.to_plan(h0.to(dev))
    lin = fm.linearize_p(Hp)
    for _ in range(3):
        Wp = torch.randn(N, 10, generator=gen).to(dev)
        Vp = torch.randn(N, 10, generator=gen).to(dev)
        got, want = lin.vjp_p(Wp), fm.vjp_p(Hp, Wp)
        assert rel_l2(got, want) < 2e-6, rel_l2(got, want)
        jv = lin.jvp_p(Vp).double()
        assert rel_l2(jv, fm.jvp_p(Hp, Vp)) < 2e-6
        lhs, rhs = float((Wp.double() * jv).sum()), float((got.double() * Vp.double()).sum())
        assert abs(lhs - rhs) <= 1e-6 * float(Wp.double().norm()) * float(jv.norm()), (lhs, rhs)
    lin.close()


def test_lin_vjp_duplicate_edges_with_mirrored_reverse(dev):
    """A duplicated edge whose reverse edge carries the mirrored attributes: the plan stores the pair as a merged slot on one side
    of one copy and as one-directional slots on the other side, so the two mask sets of one pair come from different slots of the
    neighbour's row.  The transposed product must still be the tiled VJP and the transpose of lin.jvp_p."""
    data = pkg("data")
    sd = load_weights("dirichlet")
    gen = torch.Generator().manual_seed(12)
    N = 5
    base = dict(x=torch.zeros(N, 1), y=torch.zeros(N, 1), sol=torch.zeros(N, 1), prb_data=torch.randn(N, 2, generator=gen),
                tags=torch.tensor([[1.], [0.], [0.], [0.], [1.]]), pos=torch.zeros(N, 2))

    def mirror(a):
        return torch.stack([-a[0], -a[1], a[2]])

    a, b, c = (torch.randn(3, generator=gen) for _ in range(3))
    graphs = [
        # 1 -> 2 twice (same attr), 2 -> 1 once (mirrored): the small case
        ([(1, 2, a), (1, 2, a), (2, 1, mirror(a))]),
        # the other orientation, plus a plain mirrored pair and edges to and from a Dirichlet row
        ([(2, 1, b), (1, 2, mirror(b)), (2, 1, b), (3, 2, c), (2, 3, mirror(c)), (0, 1, a), (1, 4, b), (4, 3, c)]),
        # three copies one way, two the other
        ([(1, 3, a), (3, 1, mirror(a)), (1, 3, a), (3, 1, mirror(a)), (1, 3, a), (2, 3, b)]),
    ]
    for edges in graphs:
        ei = torch.tensor([[s for s, _, _ in edges], [t for _, t, _ in edges]])
        ea = torch.stack([e for _, _, e in edges])
        m = data.MeshData(edge_index=ei, edge_attr=ea, a_ij=torch.randn(ei.shape[1], 1, generator=gen), **base)
        _check_against_tiled_vjp(m, sd, dev, gen)


def test_lin_vjp_mesh_with_duplicated_edges(dev):
    """hex13 with every seventh edge stored twice (same attributes; the reverse edge of a mesh edge is its mirror)."""
    data = pkg("data")
    g, mesh = load_case("hex13_dirichlet_s0")
    sd = load_weights("dirichlet")
    sel = torch.arange(0, mesh.edge_index.shape[1], 7)
    fields = {k: getattr(mesh, k) for k in ("x", "y", "sol", "prb_data", "tags", "pos")}
    m = data.MeshData(edge_index=torch.cat([mesh.edge_index, mesh.edge_index[:, sel]], 1),
                      edge_attr=torch.cat([mesh.edge_attr, mesh.edge_attr[sel]], 0),
                      a_ij=torch.cat([mesh.a_ij, mesh.a_ij[sel]], 0), **fields)
    _check_against_tiled_vjp(m, sd, dev, torch.Generator().manual_seed(13))


def test_validation_diagnostics_share_one_linearisation(dev, tmp_path, monkeypatch):
    """train_forward without gradients (validation): the Jacobian estimate and the logged power method use ONE linearisation at H*."""
    eng = pkg("engine")
    g, mesh, md, sd, fmap = bind("hex13_dirichlet_s0", dev)
    net = _model(sd, dev, bw_linearize=True, path_logs=str(tmp_path)).eval()
    builds = []
    orig = eng.Linearization.build
    monkeypatch.setattr(eng.Linearization, "build", lambda self, Hp: (builds.append(1), orig(self, Hp))[1])
    h0 = torch.from_numpy(g["h0"]).to(dev)
    with torch.no_grad():
        _, jl = net.deqdss.train_forward(h0, md, generator=torch.Generator(device=dev).manual_seed(1))
    assert len(builds) == 1, len(builds)
    assert torch.isfinite(jl) and float(jl) > 0
    assert (tmp_path / "spectral_radius.csv").exists()
