"""GPU: the stored linearisation of the mixed family WITH its Neumann rows (``Linearization(fmap, neumann="stored")``,
psignn_lin_create_opts in csrc/fgnn_tile_lin.hip): one linear operator on every tile, its exact transpose, float64 parity per row
class, operator properties and the consumers (adjoint solve, training step, Newton-Krylov).

Cases: the fixture hex13_mixed_s1 (547 nodes, 36 Neumann) at the natural tile size and at tile_target 64 / 128 / 192, and the
generated meshes make_hex_problem(60 / 182 / 440, mixed=True) (10 981 / 99 919 / 582 121 nodes).  Every case first proves, from the
plan's own arrays, that it reaches the branches it is meant to test (tile_classes): (a) a tile with Neumann nodes of its own, and on
the generated meshes (b) a tile with none of its own but one in its halo and (c) a tile with none among tile + halo.  Measured (own,
halo only, none): hex182 (34, 1, 356), hex440 (77, 3, 2194) -- but hex60 at the natural tile size (12, 0, 31): its 43 tiles happen to
cut the boundary so that every tile next to a Neumann node also owns one.  That plan is kept (it asserts (a) and (c), and that its
(b) is really empty), and the same mesh at tile_target 192 -- (13, 2, 43) -- is added as a case of its own so that the halo-only
branch of the transposed product is tested at this size too, with every check the other cases get."""
import functools

import numpy as np
import pytest
import torch

from conftest import CASES, load_case, load_weights, pkg, rel_l2
from oracle import psignn_oracle as orc

pytestmark = pytest.mark.gpu

FIX = "hex13_mixed_s1"
# (id, fixture tile_target or None, make_hex_problem (n, seed) or None, expected nodes)
CASE_LIST = [("hex13", 0, None, 547), ("hex13_t64", 64, None, 547), ("hex13_t128", 128, None, 547), ("hex13_t192", 192, None, 547),
             ("hex60", 0, (60, 3), 10981), ("hex60_t192", 192, (60, 3), 10981), ("hex182", 0, (182, 0), 99919), ("hex440", 0, (440, 2), 582121)]
IDS = [c[0] for c in CASE_LIST]
HALO_CAP = 512


def _to64(sd, mesh):
    m64 = mesh.clone()
    for k, v in list(vars(mesh).items()):
        if torch.is_tensor(v) and v.is_floating_point():
            setattr(m64, k, v.double())
    return {k: v.double() for k, v in sd.items()}, m64


class Case:
    def __init__(self, cid, dev):
        _, target, gen, nodes = next(c for c in CASE_LIST if c[0] == cid)
        eng, data = pkg("engine"), pkg("data")
        self.id, self.dev, self.eng = cid, dev, eng
        self.sd = sd = load_weights("mixed")
        if gen is None:
            self.g, self.mesh = load_case(FIX)
            h0 = torch.from_numpy(self.g["h0"])
        else:
            self.g, self.mesh = None, data.make_hex_problem(gen[0], seed=gen[1], mixed=True, compute_sol=False)
            with torch.no_grad():
                h0 = orc.encoder(sd, self.mesh.x)
        assert self.mesh.num_nodes == nodes
        self.N = nodes
        self.md = md = self.mesh.to(dev)
        self.plan = eng.MeshPlan(md, tile_target=target) if target else (eng.plan_for(md) if gen is None else eng.MeshPlan(md))
        self.halo_only = cid != "hex60"     # (see the module docstring)
        self.h0 = h0
        self.fmap = eng.FixedPointMap(self.plan, eng.PackedWeights(sd, dev), h0.to(dev), md.prb_data, md.unit_normal_vector)
        assert self.plan.tiled and self.plan.mixed and self.fmap.can_linearize()
        self.big = nodes >= 10000

    @functools.cached_property
    def classes(self):
        """Row classes in the caller's order: 0 = Neumann row, 1 = has a Neumann neighbour, 2 = the rest (Dirichlet rows included)."""
        fl = self.plan.export("node_flags").astype(np.int64)
        neu = ((fl & 3) == 2)
        src, dst = self.mesh.edge_index[0].numpy(), self.mesh.edge_index[1].numpy()
        near = np.zeros(self.N, bool)
        near[src[neu[dst]]] = True
        near[dst[neu[src]]] = True
        cls = np.full(self.N, 2)
        cls[near] = 1
        cls[neu] = 0
        return torch.from_numpy(cls), fl

    def tile_classes(self):
        """(tiles with Neumann nodes of their own, tiles with none of their own but one in the halo, tiles with none at all),
        from the plan's arrays."""
        cls, fl = self.classes
        perm = self.plan.export("perm").astype(np.int64)            # perm[new] = old
        neu_p = ((fl & 3) == 2)[perm]
        tp, hc = self.plan.export("tile_ptr").astype(np.int64), self.plan.export("halo_cnt").astype(np.int64)
        halo = self.plan.export("halo").astype(np.int64).reshape(-1, HALO_CAP)
        own = np.array([neu_p[tp[t]:tp[t + 1]].any() for t in range(len(hc))])
        inh = np.array([neu_p[halo[t, :hc[t]]].any() for t in range(len(hc))])
        return int(own.sum()), int((~own & inh).sum()), int((~own & ~inh).sum())

    def assert_reaches_branches(self):
        a, b, c = self.tile_classes()
        cls, _ = self.classes
        assert int((cls == 0).sum()) > 0 and a >= 1, (self.id, a, b, c)
        if self.big:
            assert c >= 1 and (b >= 1 if self.halo_only else b == 0), (self.id, a, b, c)
        return a, b, c

    def states(self):
        """Two states (caller's order, on the device): f1 of the fixture / f(f(h0)), and two further steps on."""
        fm = self.fmap
        if self.g is not None:
            s1 = fm.to_plan(torch.from_numpy(self.g["f1"]).to(self.dev))
        else:
            s1 = fm.fp(fm.fp(fm.to_plan(fm.h0)))
        s2 = fm.fp(fm.fp(s1))
        return [s1, s2]

    def stored(self):
        return self.eng.Linearization(self.fmap, neumann="stored")

    def direct(self):
        return self.eng.Linearization(self.fmap, neumann="direct")


_CACHE = {}


def case(cid, dev):
    if cid not in _CACHE:
        _CACHE.clear()          # one big mesh at a time
        _CACHE[cid] = Case(cid, dev)
    return _CACHE[cid]


def adjoint_gap(lin, Wp, Vp):
    """|<w, J v> - <J^T w, v>| / (|w| |J v|), accumulated in float64 (as tests/test_gpu_lin_vjp.py)."""
    jv = lin.jvp_p(Vp).double()
    jtw = lin.vjp_p(Wp).double()
    lhs = float((Wp.double() * jv).sum())
    rhs = float((jtw * Vp.double()).sum())
    return abs(lhs - rhs) / (float(Wp.double().norm()) * float(jv.norm()))


def class_errors(got, want64, cls):
    """rel-L2 of all rows and of each row class (nan-free: a class whose reference rows are all 0 reports its absolute norm)."""
    got, want64 = got.detach().cpu().double(), want64.double()
    out = {}
    for name, sel in (("all", torch.ones_like(cls, dtype=torch.bool)), ("neumann", cls == 0), ("near", cls == 1), ("rest", cls == 2)):
        d, w = float((got[sel] - want64[sel]).norm()), float(want64[sel].norm())
        out[name] = d / w if w > 0 else d
    return out


def parity(c, lin, Hp, seed):
    """{product: {row class: (e_stored, e_direct)}} against the float64 oracle at plan-order state Hp."""
    fm = c.fmap
    s64, m64 = _to64(c.sd, c.mesh)
    gen = torch.Generator().manual_seed(seed)
    v = torch.randn(c.N, 10, generator=gen)
    h = fm.from_plan(Hp).cpu()
    Vp = fm.to_plan(v.to(c.dev))
    cls, _ = c.classes
    res = {}
    with torch.no_grad():
        want_j = orc.function_jvp(s64, h.double(), c.h0.double(), m64, v.double())
    want_v = orc.function_vjp(s64, h.double(), c.h0.double(), m64, v.double())
    for prod, want, stored, direct in (("jvp", want_j, lin.jvp_p(Vp), fm.jvp_p(Hp, Vp)), ("vjp", want_v, lin.vjp_p(Vp), fm.vjp_p(Hp, Vp))):
        es, ed = class_errors(fm.from_plan(stored), want, cls), class_errors(fm.from_plan(direct), want, cls)
        res[prod] = {k: (es[k], ed[k]) for k in es}
    return res


def assert_parity(c, res, where):
    for prod, per in res.items():
        for k, (es, ed) in per.items():
            print(f"parity {c.id} {where} {prod} {k}: stored {es:.3e} direct {ed:.3e}")
    for prod, per in res.items():
        for k, (es, ed) in per.items():
            assert es <= 2 * ed + 1e-7, (c.id, where, prod, k, es, ed)
            if not c.big:
                assert es <= 1e-5, (c.id, where, prod, k, es)


# ------------------------------------------------------------------------------------------------------------------ 1, 2
def test_neumann_stored_flag(dev):
    c = case("hex13", dev)
    c.assert_reaches_branches()
    s, d = c.stored(), c.direct()
    assert s.neumann_stored is True and d.neumann_stored is False
    assert c.eng.Linearization(c.fmap).neumann_stored is False
    assert c.fmap.linearize_p(c.states()[0], neumann="stored").neumann_stored is True
    # no state copies in the stored handle: slot dwords + records + the tile list
    assert s.bytes < d.bytes and d.bytes - s.bytes == c.N * 15 * 4 - 8 * ((c.plan.n_tiles + 7) // 8) * 4
    g, mesh = load_case("hex13_dirichlet_s0")
    md = mesh.to(dev)
    fmd = c.eng.FixedPointMap(c.eng.plan_for(md), c.eng.PackedWeights(load_weights("dirichlet"), dev),
                              torch.from_numpy(g["h0"]).to(dev), md.prb_data)
    a, b = c.eng.Linearization(fmd, neumann="stored"), c.eng.Linearization(fmd)
    assert a.neumann_stored is False and b.neumann_stored is False and a.bytes == b.bytes
    Hp = fmd.to_plan(torch.from_numpy(g["f1"]).to(dev))
    Vp = torch.randn(mesh.num_nodes, 10, generator=torch.Generator().manual_seed(1)).to(dev)
    fmd.linearize_p(Hp, a), fmd.linearize_p(Hp, b)
    assert torch.equal(a.jvp_p(Vp), b.jvp_p(Vp)) and torch.equal(a.vjp_p(Vp), b.vjp_p(Vp))
    with pytest.raises(ValueError):
        c.eng.Linearization(c.fmap, neumann="bogus")
    with pytest.raises(ValueError):
        c.fmap.linearize_p(c.states()[0], neumann="bogus")


@pytest.mark.parametrize("cid", ["hex13", "hex60"])
def test_launch_records(cid, dev):
    """A stored handle launches no direct tile kernel; a ``"direct"`` handle launches what it always did."""
    nat = pkg("_native")
    c = case(cid, dev)
    c.assert_reaches_branches()
    Hp = c.states()[0]
    Vp = torch.randn(c.N, 10, generator=torch.Generator().manual_seed(1)).to(dev)
    s, d = c.stored(), c.direct()
    c.fmap.fp(Hp), c.plan.workspace()
    nat.prof_enable(True)
    nat.prof_collect()
    s.build(Hp), s.jvp_p(Vp), s.vjp_p(Vp)
    ran_s = nat.prof_collect()
    s.jvp_p(Vp), s.vjp_p(Vp)
    ran_s2 = nat.prof_collect()
    d.build(Hp), d.jvp_p(Vp), d.vjp_p(Vp)
    ran_d = nat.prof_collect()
    nat.prof_enable(False)
    print("stored:", sorted(ran_s), "again:", sorted(ran_s2), "direct:", sorted(ran_d))
    assert not [k for k in ran_s if k.startswith("k_jvp_tile") or k.startswith("k_vjp_tile")], ran_s
    assert {"k_lin_build_neu", "k_jvp_lin_neu", "k_vjp_lin_mixed", "k_lin_rev", "k_lin_tfill"} <= set(ran_s), ran_s
    # products only: J v one launch per tile group of the plan, J^T w one launch
    assert {"k_jvp_lin_neu", "k_vjp_lin_mixed"} <= set(ran_s2) <= {"k_jvp_lin", "k_jvp_lin_neu", "k_vjp_lin_mixed"}, ran_s2
    assert all(v[0] == 1 for v in ran_s2.values()), ran_s2
    want_d = {"k_jvp_tile", "k_vjp_tile_a", "k_vjp_tile_b"} | ({"k_lin_build", "k_jvp_lin"} if c.tile_classes()[0] < c.plan.n_tiles else set())
    assert set(ran_d) == want_d, (ran_d, want_d)


# ------------------------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("cid", IDS)
def test_transpose(cid, dev):
    """<w, J v> = <J^T w, v> to 1e-6 for the stored handle (four Gaussian pairs); the ``"direct"`` handle's gap on the same pairs is
    printed, not asserted (its two products are not one operator)."""
    c = case(cid, dev)
    print("tile classes (own, halo only, none):", c.assert_reaches_branches())
    Hp = c.states()[0]
    s, d = c.stored().build(Hp), c.direct().build(Hp)
    gen = torch.Generator().manual_seed(11)
    gaps = []
    for _ in range(4):
        Wp = torch.randn(c.N, 10, generator=gen).to(dev)
        Vp = torch.randn(c.N, 10, generator=gen).to(dev)
        gaps.append((adjoint_gap(s, Wp, Vp), adjoint_gap(d, Wp, Vp)))
    print(f"transpose gap {cid}: stored {[f'{a:.2e}' for a, _ in gaps]} direct {[f'{b:.2e}' for _, b in gaps]}")
    for a, _ in gaps:
        assert a <= 1e-6, (cid, gaps)
    s.close(), d.close()


# ------------------------------------------------------------------------------------------------------------------ 4
@pytest.mark.parametrize("cid", IDS)
def test_parity_against_float64(cid, dev):
    """lin.jvp_p / lin.vjp_p of the stored handle against the float64 oracle at two states, all rows and per row class (Neumann rows,
    rows with a Neumann neighbour, the rest): e_stored <= 2 e_direct + 1e-7, e_direct = the direct tiled kernel's error on the same
    inputs; on the fixture also e_stored <= 1e-5."""
    c = case(cid, dev)
    c.assert_reaches_branches()
    lin = c.stored()
    for i, Hp in enumerate(c.states()):
        lin.build(Hp)
        assert_parity(c, parity(c, lin, Hp, 30 + i), f"state{i}")
    lin.close()


# ------------------------------------------------------------------------------------------------------------------ 5
@pytest.mark.parametrize("cid", ["hex13", "hex13_t64", "hex60", "hex60_t192"])
def test_operator_properties(cid, dev):
    nat = pkg("_native")
    c = case(cid, dev)
    c.assert_reaches_branches()
    fm = c.fmap
    Hp = c.states()[0]
    lin = c.stored()
    gen = torch.Generator().manual_seed(2)
    Wp = torch.randn(c.N, 10, generator=gen).to(dev)
    for prod in (lin.jvp_p, lin.vjp_p):
        with pytest.raises(nat.NativeError):
            prod(Wp)                          # before any build
    fm.linearize_p(Hp, lin)
    for prod in (lin.jvp_p, lin.vjp_p):
        with pytest.raises(nat.NativeError):
            prod(Wp, out=Wp)                  # in place
        U = torch.roll(Wp, 5, 0).contiguous()
        comb = prod(1.5 * Wp - 0.25 * U)
        assert rel_l2(comb, 1.5 * prod(Wp) - 0.25 * prod(U)) < 2e-6
        a = prod(Wp)
        assert torch.equal(a, prod(Wp))
        out = torch.empty_like(Wp)
        assert prod(Wp, out=out) is out and torch.equal(out, a)
    a_j, a_v = lin.jvp_p(Wp), lin.vjp_p(Wp)
    # Dirichlet rows: J v is exactly 0 there, and they carry no cotangent
    _, fl = c.classes
    dmask = fm.to_plan(torch.from_numpy((fl & 1).astype(np.float32)).unsqueeze(1).to(dev))
    assert 0 < float(dmask.sum()) < c.N
    assert float((a_j * dmask).abs().max()) == 0.0
    assert float(lin.vjp_p(Wp * dmask).abs().max()) == 0.0
    # a rebuild at another state: that state's products (float64 rule of the parity test), not the old ones
    H2 = fm.fp(fm.fp(Hp))
    assert fm.linearize_p(H2, lin) is lin
    assert not torch.equal(lin.jvp_p(Wp), a_j) and not torch.equal(lin.vjp_p(Wp), a_v)
    assert_parity(c, parity(c, lin, H2, 40), "rebuilt")
    lin.close()


# ------------------------------------------------------------------------------------------------------------------ 6
def test_adjoint_solve_through_stored_linearisation(dev):
    """tests/test_gpu_lin_vjp.py::test_adjoint_solve_through_linearisation with a stored handle, its tolerances."""
    c = case("hex13", dev)
    c.assert_reaches_branches()
    fm, g = c.fmap, c.g
    h_star = torch.from_numpy(g["broyden_e7_result"])
    grad = torch.randn(h_star.shape, generator=torch.Generator().manual_seed(9))
    lin = fm.linearize_p(fm.to_plan(h_star.to(dev)), neumann="stored")
    assert lin.neumann_stored
    sv = c.eng.DeviceBroyden(fm.plan, 600, keep_trace=False)
    out = sv.solve_adjoint(fm, h_star.to(dev), grad.to(dev), 1e-6, lin=lin)
    assert out["lowest"] < 1e-6
    y = out["result"]
    r = orc.function_vjp(c.sd, h_star, c.h0, c.mesh, y.cpu()) + grad - y.cpu()
    assert float(r.norm() / y.cpu().norm()) < 1e-4
    base = sv.solve_adjoint(fm, h_star.to(dev), grad.to(dev), 1e-6)
    assert rel_l2(y, base["result"]) < 1e-3
    lin.close()


def _model(sd, dev, **kw):
    solver = pkg("utilities.solver")
    cfg = dict(latent_dim=10, n_layers=1, solver=solver.broyden, fw_tol=1e-7, fw_thres=600, bw_tol=1e-6, bw_thres=600)
    cfg.update(kw)
    net = pkg("mixed").ModelDEQDSS(cfg)
    net.load_state_dict(sd)
    return net.to(dev)


def test_training_step_with_stored_neumann_rows(dev):
    """One training step with bw_linearize=True, lin_neumann="stored" against the default path (the bounds of
    test_training_step_gradients_with_linearised_backward), and the model's diagnostics through a stored handle."""
    g, mesh = load_case(FIX)
    sd = load_weights("mixed")
    grads = []
    for kw in ({}, dict(bw_linearize=True, lin_neumann="stored")):
        net = _model(sd, dev, fw_tol=1e-7, fw_thres=600, bw_tol=1e-7, bw_thres=400, **kw).train()
        torch.manual_seed(0)
        u, ld = net(mesh.to(dev))
        loss = ld["residual_loss"] + ld["encoder_loss"] + ld["autoencoder_loss"]
        loss.backward()
        assert net.deqdss.last_backward["lowest"] < 1e-7
        grads.append({k: p.grad.detach().double().cpu() for k, p in net.named_parameters()})
        if kw:
            assert net.deqdss._bw_lin.neumann_stored is True
    scale = max(float(t.norm()) for t in grads[0].values())
    worst = max(float((grads[1][k] - w).norm()) / max(float(w.norm()), 1e-4 * scale) for k, w in grads[0].items())
    print("worst relative parameter-gradient difference:", worst)
    assert worst < 1e-2, worst
    # power method / Jacobian estimate through the stored handle (bounds of test_model_opt_in_backward_routes)
    md = mesh.to(dev)
    h_star = torch.from_numpy(g["broyden_e7_result"]).to(dev)
    h0 = torch.from_numpy(g["h0"]).to(dev)
    ref, st = _model(sd, dev), _model(sd, dev, bw_linearize=True, lin_neumann="stored")
    gen = torch.Generator().manual_seed(21)
    probes = [torch.randn(h_star.shape, generator=gen).to(dev) for _ in range(3)]
    ja, jb = ref.deqdss.jac_loss_estimate(h_star, h0, md, probes=probes), st.deqdss.jac_loss_estimate(h_star, h0, md, probes=probes)
    assert abs(float(jb) - float(ja)) < 1e-5 * float(ja)
    v0 = torch.randn(h_star.shape, generator=gen).to(dev)
    ea, ra = ref.deqdss.power_method(h_star, h0, md, n_iters=40, v0=v0)
    eb, rb = st.deqdss.power_method(h_star, h0, md, n_iters=40, v0=v0)
    assert abs(float(rb) - float(ra)) < 2e-4 * float(ra)
    assert st.deqdss._bw_lin.neumann_stored is True
    # lin_neumann is ignored for the dirichlet family
    gd, meshd = load_case("hex13_dirichlet_s0")
    cfg = dict(latent_dim=10, n_layers=1, bw_linearize=True, lin_neumann="stored")
    nd = pkg("model_psignn").ModelDEQDSS(cfg)
    nd.load_state_dict(load_weights("dirichlet"))
    nd = nd.to(dev)
    hd = torch.from_numpy(gd["h0"]).to(dev)
    fmd = nd.deqdss.f.bind(hd, meshd.to(dev))
    assert nd.deqdss._linearization(fmd, torch.from_numpy(gd["f1"]).to(dev)).neumann_stored is False


def test_newton_krylov_takes_the_maps_setting(dev, monkeypatch):
    """utilities.solver.newton_krylov creates its Linearization through ``f.linearize_p(x, lin)``: with the map's
    ``lin_neumann = "stored"`` the handle stores the Neumann rows, and the run agrees with the ``"direct"`` map's.
    tests/test_gpu_fpiter_krylov.py tests the GMRES machinery, not a newton_krylov result; the tolerance here is the one
    tests/test_gpu_configs.py::test_linearised_jvp_on_many_tiles_and_in_newton_krylov applies between that solver's runs with two
    Jacobian routes: the first two relative residuals to 2e-2, the same Krylov steps in the first Newton step, final residuals
    of one order (0.3 .. 3)."""
    solver, eng = pkg("utilities.solver"), pkg("engine")
    c = case("hex13", dev)
    c.assert_reaches_branches()
    made = []
    orig = eng.Linearization.__init__

    def spy(self, fmap, neumann="direct"):
        orig(self, fmap, neumann=neumann)
        made.append(self.neumann_stored)
    monkeypatch.setattr(eng.Linearization, "__init__", spy)
    outs = {}
    for mode in ("direct", "stored"):
        fm = eng.FixedPointMap(c.plan, c.fmap.weights, c.fmap.h0, c.fmap.prb, c.fmap.nrm)
        if mode == "stored":
            fm.lin_neumann = "stored"
        outs[mode] = solver.newton_krylov(fm, fm.h0, threshold=8, eps=1e-6, inner_m=40, warm_start=40)
    assert made == [False, True], made
    a, b = outs["stored"], outs["direct"]
    print("NK stored / direct:", a["rel_trace"], b["rel_trace"], a["n_krylov"], b["n_krylov"])
    np.testing.assert_allclose(a["rel_trace"][:2], b["rel_trace"][:2], rtol=2e-2)
    assert a["n_krylov"][0] == b["n_krylov"][0]
    assert 0.3 < a["lowest"] / b["lowest"] < 3.0


def test_degenerate_mixed_graphs(dev):
    """No Neumann node at all; every boundary node Neumann; an isolated Neumann node; self loops only: the stored handle builds and
    applies without error and matches the direct kernels to 2e-6 (the bound of test_lin_vjp_degenerate_graphs)."""
    eng, data = pkg("engine"), pkg("data")
    sd = load_weights("mixed")
    gen = torch.Generator().manual_seed(7)
    meshes = []
    for which in ("none", "all"):
        m = data.make_hex_problem(6, seed=4, mixed=True, compute_sol=False)
        tags = m.tags.clone()
        bnd = (tags[:, 1] + tags[:, 2]) > 0
        if which == "none":       # Neumann nodes become interior nodes
            tags[:, 0] = torch.where(tags[:, 2] > 0, torch.ones_like(tags[:, 0]), tags[:, 0])
            tags[:, 2] = 0
        else:                     # the whole boundary ring Neumann
            tags[bnd] = torch.tensor([0., 0., 1.], dtype=tags.dtype)
        m.tags = tags
        meshes.append((which, m))
    N = 6

    def small(ei, tags):
        nrm = torch.nn.functional.normalize(torch.randn(N, 2, generator=gen), dim=1)
        return data.MeshData(x=torch.zeros(N, 1), y=torch.zeros(N, 1), sol=torch.zeros(N, 1), prb_data=torch.randn(N, 3, generator=gen),
                             tags=tags, pos=torch.zeros(N, 2), edge_index=ei, edge_attr=torch.randn(ei.shape[1], 3, generator=gen),
                             a_ij=torch.randn(ei.shape[1], 1, generator=gen), unit_normal_vector=nrm)
    I, Dn, Ne = [1., 0., 0.], [0., 1., 0.], [0., 0., 1.]
    meshes.append(("isolated", small(torch.tensor([[0, 1, 2, 3, 1], [1, 2, 3, 0, 0]]), torch.tensor([Dn, I, I, Ne, I, Ne]))))   # 4, 5 isolated
    meshes.append(("selfloops", small(torch.tensor([[0, 1, 2, 3, 4, 5], [0, 1, 2, 3, 4, 5]]), torch.tensor([Dn, I, Ne, Ne, I, Dn]))))
    n_lin = 0
    for which, m in meshes:
        md = m.to(dev)
        plan = eng.MeshPlan(md)
        h0 = torch.randn(m.num_nodes, 10, generator=gen)
        fm = eng.FixedPointMap(plan, eng.PackedWeights(sd, dev), h0.to(dev), md.prb_data, md.unit_normal_vector)
        if not fm.can_linearize():
            continue
        n_lin += 1
        Hp = fm.to_plan(h0.to(dev))
        lin = fm.linearize_p(Hp, neumann="stored")
        assert lin.neumann_stored
        for _ in range(2):
            Wp = torch.randn(m.num_nodes, 10, generator=gen).to(dev)
            for got, want in ((lin.jvp_p(Wp), fm.jvp_p(Hp, Wp)), (lin.vjp_p(Wp), fm.vjp_p(Hp, Wp))):
                assert bool(torch.isfinite(got).all()), which
                assert rel_l2(got, want) < 2e-6 or float((got - want).abs().max()) == 0.0, (which, rel_l2(got, want))
        lin.close()
    assert n_lin >= 2, n_lin
