"""Every tile kernel on plans at the tile builder's structure limits (tests/limit_graphs.py), against the CPU oracle in float64.

The real meshes never come near the limits (at most 366 LDS rows per tile), so the third LDS staging pass (rows 512..767), a
255-row slot walk, 4 096 halo candidates and dynamic LDS requests near their budget are exercised here only.  Per case:

* the plan tiles or falls back as the case expects, and a tiled plan's halo, slice_deg and ELL slots are bit-exact against the
  numpy statement (tests/plan_ref.py), max_tile_rows as constructed;
* each product that runs on the plan is compared tile by tile with the float64 oracle: e_t <= max(16 e32_t, tau_op)
  (limit_graphs.check_tiles; e32_t: the float32 oracle's own error on the same tile, tau_op: the whole-vector gate of the
  fixture tests of that product), parameter gradients tensor by tensor with the same rule;
* the tiled result against an untiled plan of the same graph, at the same tolerance.

Lines starting with LIMITS report the worst per-tile error of each product and the float32 oracle's on that tile."""
import os

import numpy as np
import pytest
import torch

import limit_graphs as lg
from conftest import GOLDEN, load_case, load_weights, pkg, rel_l2
from oracle import psignn_oracle as orc
from plan_ref import tile_reference

pytestmark = pytest.mark.gpu

TAU = {"f": 2e-6, "jvp": 1e-5, "vjp": 2e-5, "pgrad": 1e-4, "pgrad_h": 2e-5, "jr": 1e-4, "jr_h": 1e-4,
       "dsgps": 2e-6, "dsgps_bw": 2e-5, "dss": 2e-6, "dss_bw": 2e-5, "dss_pgrad": 1e-4}
FAMILIES = [False, True]


def _to64(sd, mesh):
    m64 = mesh.clone()
    for k, v in list(vars(mesh).items()):
        if torch.is_tensor(v) and v.is_floating_point():
            setattr(m64, k, v.double())
    return {k: v.double() for k, v in sd.items()}, m64


def _random_two_layer(seed=5):
    torch.manual_seed(seed)
    net = pkg("model_psignn").ModelPSIGNN(dict(latent_dim=10, n_layers=2))
    for p in net.parameters():
        if p.dim() == 1:
            torch.nn.init.normal_(p, std=0.1)
    return {k: v.detach().clone() for k, v in net.state_dict().items()}


class Run:
    """One case in one family: the plan under test, an untiled plan of the same graph, inputs, and the report."""

    def __init__(self, name, mixed, dev):
        self.case = c = lg.build(name, mixed)
        self.name, self.mixed, self.dev = f"{name}-{'mixed' if mixed else 'dirichlet'}", mixed, dev
        self.m = c.mesh
        self.md = c.mesh.to(dev)
        self.N = N = c.mesh.num_nodes
        eng = self.eng = pkg("engine")
        self.plan = eng.MeshPlan(self.md, tile_target=c.tile_target)
        self.sd = load_weights("mixed" if mixed else "dirichlet")
        self.w = eng.PackedWeights(self.sd, dev)
        gen = torch.Generator().manual_seed(21)
        self.h0, self.h, self.v, self.wv, self.gb = (0.3 * torch.randn(N, 10, generator=gen) for _ in range(5))
        self.gb /= N
        self.nrm = getattr(self.md, "unit_normal_vector", None)
        self.fm = eng.FixedPointMap(self.plan, self.w, self.h0.to(dev), self.md.prb_data, self.nrm)
        self.s64, self.m64 = _to64(self.sd, self.m)
        if self.plan.tiled:
            self.perm, self.tile_ptr = self.plan.export("perm"), self.plan.export("tile_ptr")
        else:
            self.perm, self.tile_ptr = np.arange(N), lg.chunk_tiles(N)
        self.named = []
        self.report = {}

    def dev_(self, t):
        return t.to(self.dev)

    def check(self, op, got, want64, want32, tau):
        e, e32 = lg.check_tiles(got, want64, want32, self.perm, self.tile_ptr, tau, f"{self.name} {op}", self.named)
        et = lg.tile_errors(got, want64, self.perm, self.tile_ptr)
        named = {t: float(et[t]) for t in self.named}
        self.report[op] = (e, e32)
        print(f"LIMITS {self.name} {op}: worst tile {e:.2e} (fp32 oracle {e32:.2e}) named {named}")

    def check_params(self, op, got, want64, want32, tau):
        worst = lg.check_params(got, want64, want32, tau, f"{self.name} {op}")
        self.report[op] = worst
        print(f"LIMITS {self.name} {op}: worst tensor {worst[0]:.2e} (fp32 oracle {worst[1]:.2e})")


def _check_structures(r):
    c, plan = r.case, r.plan
    assert plan.tiled == c.tiled, (r.name, plan.tiled)
    if not plan.tiled:
        assert plan.max_tile_rows == 0
        return
    m = r.m
    perm, tile_ptr = r.perm, r.tile_ptr
    ei, ea = m.edge_index.numpy(), m.edge_attr.numpy()
    if m.pos is None:
        assert np.array_equal(perm, np.arange(r.N)) and np.array_equal(tile_ptr, lg.chunk_tiles(r.N, c.tile_target))
    ref = tile_reference(ei, r.N, perm, tile_ptr, ea)
    assert np.array_equal(plan.export("halo_cnt"), ref["halo_cnt"])
    halo = plan.export("halo").reshape(-1, lg.HALO_CAP)
    for t, h in enumerate(ref["halo"]):
        assert np.array_equal(halo[t, :len(h)], h), t
    assert np.array_equal(plan.export("slice_deg"), ref["slice_deg"])
    assert np.array_equal(plan.export("ell").reshape(-1, 64, 4), ref["ell"])
    rows = np.diff(tile_ptr) + ref["halo_cnt"]
    assert plan.max_tile_rows == int(rows.max())
    if c.max_rows is not None:
        assert plan.max_tile_rows == c.max_rows
    for t, h in c.halo_cnt.items():
        assert ref["halo_cnt"][t] == h
    for s, d in c.slice_deg.items():
        assert ref["slice_deg"][s] == d
    # the tiles checked by name: the most rows, and the one holding the deepest slot walk
    r.named = [int(np.argmax(rows))]
    if c.slot_node is not None:
        inv = np.empty(r.N, dtype=np.int64)
        inv[perm] = np.arange(r.N)
        r.named.append(int(np.searchsorted(tile_ptr, inv[c.slot_node], side="right") - 1))


def _f_products(r, knobs):
    H = r.dev_(r.h)
    with torch.no_grad():
        want = orc.function_forward(r.s64, r.h.double(), r.h0.double(), r.m64)
        want32 = orc.function_forward(r.sd, r.h.clone(), r.h0, r.m)
    got = r.fm(H)
    r.check("f", got, want, want32, TAU["f"])
    if r.plan.tiled:
        Hp = r.fm.to_plan(H)
        assert torch.equal(r.fm.from_plan(r.fm.fp(Hp)), got)
        assert torch.equal(r.fm.from_plan(r.fm.picard_p(Hp, 1)), got)
        for form in ("mfma", "valu"):
            knobs(PSIGNN_STAGE1=form)
            fm = r.eng.FixedPointMap(r.eng.MeshPlan(r.md, tile_target=r.case.tile_target), r.w, r.fm.h0, r.md.prb_data, r.nrm)
            gf = fm(H)
            r.check(f"f[{form}]", gf, want, want32, TAU["f"])
            assert torch.equal(fm.from_plan(fm.picard_p(fm.to_plan(H), 1)), gf)
            knobs(PSIGNN_STAGE1=None)
        if r.mixed:     # tiles without Neumann nodes in a launch of their own: the same bits
            knobs(PSIGNN_MIXED_SPLIT_MIN="0")
            assert torch.equal(r.fm(H), got)
            knobs(PSIGNN_MIXED_SPLIT_MIN="1000000")
            assert torch.equal(r.fm(H), got)
            knobs(PSIGNN_MIXED_SPLIT_MIN=None)
    return got


def _jvp_products(r, knobs):
    H, V = r.dev_(r.h), r.dev_(r.v)
    want = orc.function_jvp(r.s64, r.h.double(), r.h0.double(), r.m64, r.v.double())
    want32 = orc.function_jvp(r.sd, r.h, r.h0, r.m, r.v)
    got = r.fm.jvp(H, V)
    r.check("jvp", got, want, want32, TAU["jvp"])
    if r.plan.tiled:
        for form in ("mfma", "valu"):
            knobs(PSIGNN_JVP_STAGE1=form)
            jp = r.fm.from_plan(r.fm.jvp_p(r.fm.to_plan(H), r.fm.to_plan(V)))
            r.check(f"jvp_p[{form}]", jp, want, want32, TAU["jvp"])
            knobs(PSIGNN_JVP_STAGE1=None)
        assert torch.equal(r.fm.from_plan(r.fm.jvp_p(r.fm.to_plan(H), r.fm.to_plan(V))), got)
    return got, want, want32


def _vjp_products(r):
    H, W = r.dev_(r.h), r.dev_(r.wv)
    want = orc.function_vjp(r.s64, r.h.double(), r.h0.double(), r.m64, r.wv.double())
    want32 = orc.function_vjp(r.sd, r.h, r.h0, r.m, r.wv)
    got = r.fm.vjp(H, W)
    r.check("vjp", got, want, want32, TAU["vjp"])
    if r.plan.tiled:
        assert torch.equal(r.fm.from_plan(r.fm.vjp_p(r.fm.to_plan(H), r.fm.to_plan(W))), got)
    return got, want, want32


def _lin_products(r, jv, vj):
    fm = r.fm
    assert fm.can_linearize()
    Hp = fm.to_plan(r.dev_(r.h))
    lin = fm.linearize_p(Hp)
    try:
        r.check("lin.jvp_p", fm.from_plan(lin.jvp_p(fm.to_plan(r.dev_(r.v)))), jv[1], jv[2], TAU["jvp"])
        r.check("lin.vjp_p", fm.from_plan(lin.vjp_p(fm.to_plan(r.dev_(r.wv)))), vj[1], vj[2], TAU["vjp"])
    finally:
        lin.close()


def _pgrad_products(r, fm, sd, h, s64, tag=""):
    m, m64 = r.m, r.m64
    want, want_h, want_init = orc.function_param_vjp(s64, h.double(), r.h0.double(), m64, r.wv.double())
    want32, want32_h, want32_init = orc.function_param_vjp(sd, h, r.h0, m, r.wv)
    zero = lambda g, ref: {k: (torch.zeros_like(ref["deqdss.f." + k]) if t is None else t) for k, t in g.items()}
    want, want32 = zero(want, s64), zero(want32, sd)
    grads, dh, dinit = fm.param_vjp_init(r.dev_(h), r.dev_(r.wv))
    assert set(grads) == set(want)
    r.check_params(f"param_vjp{tag}", grads, want, want32, TAU["pgrad"])
    r.check(f"param_vjp{tag} dh", dh, want_h, want32_h, TAU["pgrad_h"])
    r.check(f"param_vjp{tag} dh_init", dinit, want_init, want32_init, TAU["pgrad_h"])
    if r.plan.tiled and not r.mixed:
        flat, out_p = fm.param_vjp_p(fm.to_plan(r.dev_(h)), fm.to_plan(r.dev_(r.wv)))
        named = r.eng.unpack_param_grads(flat, fm.weights.n_layers, False)
        assert all(torch.equal(named[k], grads[k]) for k in grads)
        assert torch.equal(fm.from_plan(out_p), dh)
    want, want_h, _ = orc.function_vjp_backward(s64, h.double(), r.h0.double(), m64, r.wv.double(), r.gb.double())
    want32, want32_h, _ = orc.function_vjp_backward(sd, h, r.h0, m, r.wv, r.gb)
    g2, d2 = fm.vjp_backward(r.dev_(h), r.dev_(r.wv), r.dev_(r.gb))
    r.check_params(f"vjp_backward{tag}", g2, want, want32, TAU["jr"])
    r.check(f"vjp_backward{tag} dh", d2, want_h, want32_h, TAU["jr_h"])


def _two_layer_products(r):
    """Dirichlet block with L = 2 (the LayerNorm-off instantiations on the first layer): JVP, VJP, parameter VJP, backward
    of the VJP.  The state carries h_initial's Dirichlet rows (the derivative entry points take no h_initial)."""
    sd = _random_two_layer()
    s64 = {k: v.double() for k, v in sd.items()}
    h0, h = r.h0, r.h.clone()
    idx = torch.where(r.m.tags[:, 0] == 1)[0]
    h[idx] = h0[idx]
    fm = r.eng.FixedPointMap(r.plan, r.eng.PackedWeights(sd, r.dev), r.dev_(h0), r.md.prb_data)
    H, V, W = r.dev_(h), r.dev_(r.v), r.dev_(r.wv)
    r.check("jvp L2", fm.jvp(H, V), orc.function_jvp(s64, h.double(), h0.double(), r.m64, r.v.double()),
            orc.function_jvp(sd, h, h0, r.m, r.v), TAU["jvp"])
    r.check("vjp L2", fm.vjp(H, W), orc.function_vjp(s64, h.double(), h0.double(), r.m64, r.wv.double()),
            orc.function_vjp(sd, h, h0, r.m, r.wv), TAU["vjp"])
    if r.plan.tiled:
        Hp = fm.to_plan(H)
        assert torch.equal(fm.from_plan(fm.jvp_p(Hp, fm.to_plan(V))), fm.jvp(H, V))
        assert torch.equal(fm.from_plan(fm.vjp_p(Hp, fm.to_plan(W))), fm.vjp(H, W))
    _pgrad_products(r, fm, sd, h, s64, tag=" L2")


def _dsgps_products(r):
    eng = r.eng
    wd = np.load(os.path.join(GOLDEN, "weights_dsgps_mixed.npz" if r.mixed else "weights_dsgps.npz"))
    sd = {n: torch.from_numpy(wd[n]) for n in wd.files if n != "k"}
    s64 = {k: v.double() for k, v in sd.items()}
    fm = r.fm
    H = r.dev_(r.h)
    with torch.no_grad():
        want = orc.dsgps_step(s64, r.h.double(), r.h0.double(), r.m64)
        want32 = orc.dsgps_step(sd, r.h.clone(), r.h0, r.m)
    fm.fp(fm.to_plan(H))                     # plan-order copies of h0 / prb / normals
    h0p, prbp, nrmp = fm._p
    got = fm.from_plan(eng.dsgps_step_p(r.plan, eng.pack_dsgps(sd, r.dev), fm.to_plan(H), h0p, prbp, nrmp))
    r.check("dsgps_step_p", got, want, want32, TAU["dsgps"])
    names = [k for k in sd if not k.startswith(("autoencoder", "laynorm"))]

    def grads(p_sd, h, w):
        pp = {k: (v.clone().requires_grad_(True) if k in names else v) for k, v in p_sd.items()}
        hh = h.clone().requires_grad_(True)
        m = r.m64 if h.dtype == torch.float64 else r.m
        h0 = r.h0.to(h.dtype)
        g = torch.autograd.grad(orc.dsgps_step(pp, hh, h0, m), [pp[k] for k in names] + [hh], w)
        return dict(zip(names, g[:-1])), g[-1]
    want_g, want_h = grads(s64, r.h.double(), r.wv.double())
    want32_g, want32_h = grads(sd, r.h, r.wv)
    wf, wg = eng.pack_dsgps_train(sd, r.dev)
    g3, dh3 = eng.dsgps_step_backward(r.plan, wf, wg, H, r.md.prb_data, r.dev_(r.wv), r.nrm)
    r.check_params("dsgps_step_backward", g3, want_g, want32_g, TAU["dsgps_bw"])
    r.check("dsgps_step_backward dh", dh3, want_h, want32_h, TAU["dsgps_bw"])


class _DssBatch:
    pass


def _dss_products(r):
    """DSS update t on the plan of the DSS graph (self loops dropped, edge_attr = (0, 0, a_norm)): the zero attrs are not
    mirrors bit for bit (+0 vs -0), so every edge direction is a slot of its own; the plan tiles where those limits allow."""
    eng = r.eng
    w = np.load(os.path.join(GOLDEN, "weights_dss.npz"))
    sd = {n: torch.from_numpy(w[n]) for n in w.files if n not in ("k", "alpha")}
    k, t, alpha = int(w["k"]), 3, 1.0
    gen = torch.Generator().manual_seed(8)
    ei = r.m.edge_index
    ei = ei[:, ei[0] != ei[1]]
    E = ei.shape[1]
    a_norm = torch.randn(E, 1, generator=gen)
    bpn = torch.randn(r.N, 3, generator=gen)
    view = pkg("data").MeshData(x=torch.zeros(r.N, 1), edge_index=ei, a_ij=torch.randn(E, 1, generator=gen),
                                edge_attr=torch.cat([torch.zeros(E, 2), a_norm], dim=1).contiguous(),
                                tags=torch.zeros(r.N, 1), pos=r.m.pos)
    plan = eng.MeshPlan(view.to(r.dev))
    lim = lg.limits_of(ei.numpy(), r.N, view.edge_attr.numpy(), *(
        (plan.export("perm"), plan.export("tile_ptr")) if plan.tiled else (None, None)))
    if r.m.pos is None:
        assert plan.tiled == lg.should_tile(lim, False), (r.name, "dss plan")
    if not plan.tiled:       # the DSS kernels run on tiled plans only
        print(f"LIMITS {r.name} dss: plan untiled (slots per node {int(lim['slice_deg'].max())})")
        return
    perm, tile_ptr = plan.export("perm"), plan.export("tile_ptr")
    b64, b32 = _DssBatch(), _DssBatch()
    for b, dt in ((b64, torch.float64), (b32, torch.float32)):
        b.edge_index, b.a_ij_norm, b.b_prime_norm = ei, a_norm.to(dt), bpn.to(dt)
    s64 = {n: v.double() for n, v in sd.items()}
    h = r.h
    with torch.no_grad():
        want = orc.dss_step(s64, t, h.double(), b64, alpha)
        want32 = orc.dss_step(sd, t, h, b32, alpha)
    # the update alone: h + alpha psi -- compared without h, whose bits pass through
    upd = lambda x: x - h.to(x.dtype).to(x.device)
    got = plan.permute(eng.dss_step_p(plan, eng.pack_dss(sd, k, r.dev), t, alpha, plan.permute(r.dev_(h), True),
                                      plan.permute(r.dev_(bpn), True)), False)
    e, e32 = lg.check_tiles(upd(got.cpu()), upd(want), upd(want32), perm, tile_ptr, TAU["dss"], f"{r.name} dss_step_p")
    print(f"LIMITS {r.name} dss_step_p: worst tile {e:.2e} (fp32 oracle {e32:.2e})")
    names = [n for n in sd if n.startswith((f"phi_to_list.{t}.", f"phi_from_list.{t}.", f"psi_list.{t}."))]

    def grads(p_sd, b, hh, wv):
        pp = {n: (v.clone().requires_grad_(True) if n in names else v) for n, v in p_sd.items()}
        hq = hh.clone().requires_grad_(True)
        g = torch.autograd.grad(orc.dss_step(pp, t, hq, b, alpha), [pp[n] for n in names] + [hq], wv)
        return dict(zip(names, g[:-1])), g[-1]
    want_g, want_h = grads(s64, b64, h.double(), r.wv.double())
    want32_g, want32_h = grads(sd, b32, h, r.wv)
    g, dh = eng.dss_step_backward(plan, eng.pack_dss_train(sd, t, r.dev), t, alpha, r.dev_(h), r.dev_(bpn), r.dev_(r.wv))
    r.check_params("dss_step_backward", g, want_g, want32_g, TAU["dss_pgrad"])
    e, e32 = lg.check_tiles(dh, want_h, want32_h, perm, tile_ptr, TAU["dss_bw"], f"{r.name} dss_step_backward dh")
    print(f"LIMITS {r.name} dss_step_backward dh: worst tile {e:.2e} (fp32 oracle {e32:.2e})")


def _against_untiled(r, f, jv, vj):
    """The tiled results against the global-gather kernels on an untiled plan of the same graph, at the same tolerances."""
    flat = r.eng.FixedPointMap(r.eng.MeshPlan(r.md, tile_target=-1), r.w, r.fm.h0, r.md.prb_data, r.nrm)
    assert not flat.plan.tiled
    H = r.dev_(r.h)
    for op, a, b, tau in (("f", f, flat(H), TAU["f"]), ("jvp", jv, flat.jvp(H, r.dev_(r.v)), TAU["jvp"]),
                          ("vjp", vj, flat.vjp(H, r.dev_(r.wv)), TAU["vjp"])):
        e = lg.tile_errors(a, b.double(), r.perm, r.tile_ptr)
        assert e.max() <= tau, (r.name, op, "tiled vs untiled", float(e.max()))
        print(f"LIMITS {r.name} {op} tiled vs untiled: worst tile {e.max():.2e}")


def _broyden_trace(r):
    solver = pkg("utilities.solver")
    with torch.no_grad():
        want = orc.broyden(lambda X: orc.function_forward(r.sd, X, r.h0, r.m), r.h0.clone(), threshold=5, eps=1e-12)
    got = solver.broyden(r.fm, r.fm.h0, threshold=5, eps=1e-12)
    a, b = np.array(got["rel_trace"][:5]), np.array(want["rel_trace"][:5])
    print(f"LIMITS {r.name} broyden rel_trace[:5] max rel diff {float(np.max(np.abs(a - b) / b)):.2e}")
    assert np.allclose(a, b, rtol=2e-3), (r.name, a, b)


@pytest.mark.parametrize("mixed", FAMILIES, ids=["dirichlet", "mixed"])
@pytest.mark.parametrize("name", lg.CASE_NAMES)
def test_every_kernel_at_the_plan_limits(name, mixed, dev, knobs):
    r = Run(name, mixed, dev)
    _check_structures(r)
    f = _f_products(r, knobs)
    jv = _jvp_products(r, knobs)
    vj = _vjp_products(r)
    if not r.plan.tiled:
        return          # past a limit: the global-gather kernels (f, JVP, VJP above) are what runs
    _against_untiled(r, f, jv[0], vj[0])
    _lin_products(r, jv, vj)
    _pgrad_products(r, r.fm, r.sd, r.h, r.s64)
    if not mixed:
        _two_layer_products(r)
    _dsgps_products(r)
    if not mixed:
        _dss_products(r)
    _broyden_trace(r)


def test_mixed_jvp_at_the_row_limit(dev):
    """Mixed plans tile up to 682 rows -- the Neumann tiles' JVP keeps 240 bytes per LDS row in 160 KiB -- and stay untiled
    beyond, so that jvp, jvp_p and Newton-Krylov work on every tiled mixed plan.  (Before the builder knew this limit, a 683-row
    mixed plan tiled and its jvp / jvp_p raised while f, the VJP and the solvers ran.)"""
    solver = pkg("utilities.solver")
    for name, tiled in (("jvp682", True), ("jvp683", False)):
        r = Run(name, True, dev)
        assert r.plan.tiled == tiled and r.plan.max_tile_rows == (682 if tiled else 0)
        H, V = r.dev_(r.h), r.dev_(r.v)
        want = orc.function_jvp(r.s64, r.h.double(), r.h0.double(), r.m64, r.v.double())
        assert rel_l2(r.fm.jvp(H, V), want) < TAU["jvp"]
        if tiled:
            assert rel_l2(r.fm.from_plan(r.fm.jvp_p(r.fm.to_plan(H), r.fm.to_plan(V))), want) < TAU["jvp"]
            out = solver.newton_krylov(r.fm, r.fm.h0, threshold=10, eps=1e-6, inner_m=30)
            assert np.isfinite(out["lowest"]) and out["n_feval"] > 0
            print(f"LIMITS {r.name} newton_krylov lowest {out['lowest']:.2e} after {out['n_feval']} evaluations")
        else:
            with pytest.raises(pkg("_native").NativeError):
                r.fm.jvp_p(r.fm.to_plan(H), r.fm.to_plan(V))
    # the same graph in the dirichlet family (160-byte JVP rows) tiles at 683 rows
    assert Run("jvp683", False, dev).plan.max_tile_rows == 683


def test_batched_broyden_with_a_768_row_mesh(dev):
    """psignn_broyden_solve_batch on a shard holding a 768-row plan (halo512) and a fixture mesh: k_f_tile_batch sizes its LDS
    by the shard's max_rows.  Each mesh's solve equals its own single-mesh solve bit for bit."""
    eng = pkg("engine")
    sd = load_weights("dirichlet")
    w = eng.PackedWeights(sd, dev)
    r = Run("halo512", False, dev)
    g, mesh = load_case("hex13_dirichlet_s0")
    md = mesh.to(dev)
    fm2 = eng.FixedPointMap(eng.MeshPlan(md), w, torch.from_numpy(g["h0"]).to(dev), md.prb_data)
    fm1 = eng.FixedPointMap(r.plan, w, r.fm.h0, r.md.prb_data)
    fmaps = [fm1, fm2]
    assert fm1.plan.max_tile_rows == 768 and fm2.plan.max_tile_rows < 768
    total = sum(f.plan.N for f in fmaps) * 10
    solvers = [eng.DeviceBroyden(plan=f.plan, threshold=40, keep_trace=False, shard_elems=total) for f in fmaps]
    try:
        assert eng.shard_batchable(solvers)
        single = [sv.solve(f, 1e-6) for sv, f in zip(solvers, fmaps)]
        outs = eng.broyden_solve_batch(solvers, fmaps, 1e-6)
        for a, b in zip(single, outs):
            assert a["n_iter"] == b["n_iter"] and a["nstep"] == b["nstep"] and a["rel_trace"] == b["rel_trace"]
            assert torch.equal(a["result"], b["result"])
        # the 768-row mesh's batched result against the float64 oracle's f at that state
        x = outs[0]["result"]
        with torch.no_grad():
            want = orc.function_forward(r.s64, x.cpu().double(), r.h0.double(), r.m64)
            want32 = orc.function_forward(r.sd, x.cpu().clone(), r.h0, r.m)
        r.check("f at the batched result", fm1(x), want, want32, TAU["f"])
    finally:
        for sv in solvers:
            sv.close()
