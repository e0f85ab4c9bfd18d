"""Every gradient kernel at the sizes the bench and a scaled-up training run use, against the CPU oracle in float64.

Every parameter gradient goes through one reduction (csrc/fgnn_pgrad.hip: k_pgrad_outer, then k_pgrad_reduce /
k_pgrad_reduce_acc), whose shape depends on the number of records (tests/pgrad_ref.py).  Past 262 144 records a wave owns
more than 64 of them and the last block holds ragged and empty waves; the fixture tests never get there.  Here:

* 1 000 519 nodes (make_hex_problem(577), the bench mesh): the parameter VJP in both families on the tiled plan and on an
  untiled one, its ``dh`` / ``dh_init``, the tiled VJPs (fm.vjp, vjp_p, lin.vjp_p) against the same reference, and the
  residual backward;
* 270 901 nodes (make_hex_problem(300)): the backward of the VJP (2N records) in both families, the two-layer dirichlet
  parameter VJP (k_pgrad_reduce_acc), the DS-GPS step backward in both families and the DSS step backward;
* the MLP backward at ragged lengths up to 4 194 305 rows.

State-shaped results are compared tile by tile (limit_graphs.check_tiles), parameter gradients tensor by tensor
(limit_graphs.check_params): e <= max(tau, 16 e32), e32 the float32 oracle's own error on the same quantity.  Dense
comparisons cannot see a dropped or doubled partial (about 1/1 000 of the terms), so each reduction is also probed: the
cotangent is kept only on the nodes whose records sit at a reduction boundary (the first wave, the whole last block, the
waves around a block boundary in the middle, the seam between the two record sets of the backward of the VJP) and on
their neighbours, and the result compared with the oracle on that support and its one-hop (backward of the VJP: two-hop)
neighbourhood, which is exact: f at a node reads only its one-hop neighbourhood.  A lost partial is then an O(1) error.

Lines starting with SCALE report the worst error of each product and the float32 oracle's on the same tile or tensor."""
import os
import time

import numpy as np
import pytest
import torch

import limit_graphs as lg
import pgrad_ref as pr
from conftest import GOLDEN, load_weights, pkg
from oracle import psignn_oracle as orc
from test_gpu_plan_limits import TAU as LIMIT_TAU
from test_gpu_plan_limits import _dsgps_products, _random_two_layer, _to64

pytestmark = pytest.mark.gpu

# the fixture gates of each product (test_gpu_training.py, test_gpu_plan_limits.py)
TAU = {"pgrad": 2e-5, "pgrad_h": 2e-5, "vjp": LIMIT_TAU["vjp"], "jr": 2e-4, "jr_h": 2e-4, "dsgps_bw": LIMIT_TAU["dsgps_bw"],
       "dss_bw": LIMIT_TAU["dss_bw"], "dss_pgrad": LIMIT_TAU["dss_pgrad"], "mlp": 1e-5, "residual": 1e-5}
HEX = {1000519: 577, 270901: 300}       # nodes -> make_hex_problem size
FAMILIES = [False, True]
FAMILY_IDS = ["dirichlet", "mixed"]
T0 = time.time()


def _report(what, e, e32):
    print(f"SCALE {what}: worst {e:.2e} (fp32 oracle {e32:.2e})  [{time.time() - T0:.0f} s]")


class Scale:
    """One hex mesh in one family, on its default (tiled) plan, at the state two f steps from the encoder state."""

    def __init__(self, N, mixed, dev):
        data, eng = pkg("data"), pkg("engine")
        self.eng, self.mixed, self.dev, self.N = eng, mixed, dev, N
        self.m = m = data.make_hex_problem(HEX[N], seed=0, mixed=mixed, compute_sol=False)
        assert m.num_nodes == N
        self.name = f"{N}-{'mixed' if mixed else 'dirichlet'}"
        self.md = md = m.to(dev)
        self.sd = load_weights("mixed" if mixed else "dirichlet")
        self.w = eng.PackedWeights(self.sd, dev)
        self.plan = eng.MeshPlan(md)
        assert self.plan.tiled
        self.nrm = getattr(md, "unit_normal_vector", None)
        P = "autoencoder.encoder.mlp.mlp."
        h0 = eng.mlp2(md.x, *[self.sd[P + k].to(dev) for k in ("0.weight", "0.bias", "2.weight", "2.bias")])
        self.fm = eng.FixedPointMap(self.plan, self.w, h0, md.prb_data, self.nrm)
        self.h0, self.h = h0.cpu(), self.fm(self.fm(h0)).cpu()
        gen = torch.Generator().manual_seed(21)
        self.v, self.wv, self.gb = (0.3 * torch.randn(N, 10, generator=gen) for _ in range(3))
        self.gb /= N
        self.s64, self.m64 = _to64(self.sd, m)
        self.perm, self.tile_ptr = self.plan.export("perm"), self.plan.export("tile_ptr")
        self.src, self.dst = m.edge_index[0].numpy(), m.edge_index[1].numpy()

    def dev_(self, t):
        return t.to(self.dev)

    def check(self, op, got, want64, want32, tau, perm=None, tile_ptr=None):
        perm, tile_ptr = (self.perm, self.tile_ptr) if perm is None else (perm, tile_ptr)
        e, e32 = lg.check_tiles(got, want64, want32, perm, tile_ptr, tau, f"{self.name} {op}")
        _report(f"{self.name} {op}", e, e32)

    def check_params(self, op, got, want64, want32, tau):
        e, e32 = lg.check_params(got, want64, want32, tau, f"{self.name} {op}")
        _report(f"{self.name} {op}", e, e32)

    def check_vec(self, op, got, want64, want32, tau):
        """A probe's state-shaped result, zero away from the probe: one relative error over all rows."""
        err = lambda a: float((torch.as_tensor(a).detach().cpu().double() - want64).norm()) / float(want64.norm())
        e, e32 = err(got), err(want32)
        assert e <= max(tau, 16 * e32), (f"{self.name} {op}", e, e32)
        _report(f"{self.name} {op}", e, e32)

    def hood(self, nodes, hops):
        """Boolean mask of ``nodes`` and their ``hops``-hop neighbourhood."""
        inn = np.zeros(self.N, bool)
        inn[nodes] = True
        for _ in range(hops):
            e = inn[self.src] | inn[self.dst]
            inn[self.src[e]] = True
            inn[self.dst[e]] = True
        return inn

    def sub(self, nodes, hops):
        """The graph induced by ``nodes`` and their ``hops``-hop neighbourhood: (kept node ids, float32 mesh, float64 mesh).
        Every edge at a node of ``nodes`` is kept, so what f computes on those nodes is what it computes on the whole graph."""
        inn = self.hood(nodes, hops)
        keep = np.flatnonzero(inn)
        emask = inn[self.src] & inn[self.dst]
        new = np.full(self.N, -1, np.int64)
        new[keep] = np.arange(len(keep))
        E = len(self.src)
        fields = {}
        for k, t in vars(self.m).items():
            if not torch.is_tensor(t):
                continue
            if k == "edge_index":
                fields[k] = torch.from_numpy(new[t.numpy()[:, emask]])
            elif t.shape[0] == E:
                fields[k] = t[torch.from_numpy(emask)]
            elif t.shape[0] == self.N:
                fields[k] = t[torch.from_numpy(keep)]
        m32 = type(self.m)(**fields)
        return torch.from_numpy(keep), m32, _to64({}, m32)[1]

    def support(self, nodes):
        """A probe's cotangent support: the nodes behind the probed records and their one-hop neighbours.  A node's records
        also carry its neighbours' terms, so the probed records hold terms even where their own nodes are Dirichlet nodes
        (the caller's order of a hex mesh starts and ends with boundary rings)."""
        return np.flatnonzero(self.hood(nodes, 1))

    def scatter(self, keep, rows):
        out = torch.zeros(self.N, rows.shape[1], dtype=rows.dtype)
        out[keep] = rows
        return out


@pytest.fixture(scope="module")
def scale(dev):
    """Scale objects, built once per module and size (the other size is dropped when a new one is built)."""
    cache = {}

    def get(N, mixed):
        if (N, mixed) not in cache:
            for k in [k for k in cache if k[0] != N]:
                del cache[k]
            cache[(N, mixed)] = Scale(N, mixed, dev)
        return cache[(N, mixed)]
    yield get
    cache.clear()


def _filled(g, ref):
    return {k: (torch.zeros_like(ref["deqdss.f." + k]) if t is None else t) for k, t in g.items()}


def _nonzero(what, want):
    assert max(float(t.norm()) for t in want.values()) > 0, (what, "the probe carries no term")


def _masked(t, nodes):
    out = torch.zeros_like(t)
    out[nodes] = t[nodes]
    return out


def _probe_param_vjp(r, fmap, order, tag):
    """Parameter VJP with the cotangent on the nodes behind each probe of the N records (``order``: record position ->
    node), against the oracle on the support's one-hop neighbourhood."""
    for name, pos in pr.probes(r.N).items():
        S = r.support(pr.nodes_at(pos, order, r.N))
        keep, m32, m64 = r.sub(S, 1)
        wv = _masked(r.wv, torch.from_numpy(S))
        h, h0, w = r.h[keep], r.h0[keep], wv[keep]
        want, want_h, _ = orc.function_param_vjp(r.s64, h.double(), h0.double(), m64, w.double())
        want32, want32_h, _ = orc.function_param_vjp(r.sd, h, h0, m32, w)
        grads, dh = fmap.param_vjp(r.dev_(r.h), r.dev_(wv))
        _nonzero(f"{r.name} {tag} probe [{name}]", want)
        r.check_params(f"{tag} probe [{name}]", grads, _filled(want, r.s64), _filled(want32, r.sd), TAU["pgrad"])
        r.check_vec(f"{tag} probe [{name}] dh", dh, r.scatter(keep, want_h), r.scatter(keep, want32_h), TAU["pgrad_h"])


@pytest.mark.parametrize("mixed", FAMILIES, ids=FAMILY_IDS)
def test_param_vjp_at_1m(mixed, scale):
    """1 000 519 records (npw = 248; the last block's waves hold 248, 248, 87 and 0): parameter gradients, dh and dh_init
    against fp64, the tiled VJPs against the same dh, an untiled plan of the mesh (gather records, caller's order) against
    the same reference, and the probes on both record orders."""
    r = scale(1000519, mixed)
    fm, eng = r.fm, r.eng
    H, W = r.dev_(r.h), r.dev_(r.wv)
    want, want_h, want_init = orc.function_param_vjp(r.s64, r.h.double(), r.h0.double(), r.m64, r.wv.double())
    want32, want32_h, want32_init = orc.function_param_vjp(r.sd, r.h, r.h0, r.m, r.wv)
    want, want32 = _filled(want, r.s64), _filled(want32, r.sd)
    grads, dh, dinit = fm.param_vjp_init(H, W)
    assert set(grads) == set(want)
    r.check_params("param_vjp", grads, want, want32, TAU["pgrad"])
    r.check("param_vjp dh", dh, want_h, want32_h, TAU["pgrad_h"])
    r.check("param_vjp dh_init", dinit, want_init, want32_init, TAU["pgrad_h"])
    # dh is the VJP: the tiled VJP kernels against the same reference
    Hp, Wp = fm.to_plan(H), fm.to_plan(W)
    r.check("vjp", fm.vjp(H, W), want_h, want32_h, TAU["vjp"])
    r.check("vjp_p", fm.from_plan(fm.vjp_p(Hp, Wp)), want_h, want32_h, TAU["vjp"])
    assert fm.can_linearize()
    lin = fm.linearize_p(Hp)
    try:
        r.check("lin.vjp_p", fm.from_plan(lin.vjp_p(Wp)), want_h, want32_h, TAU["vjp"])
    finally:
        lin.close()
    if not mixed:
        flat, out_p = fm.param_vjp_p(Hp, Wp)
        named = eng.unpack_param_grads(flat, fm.weights.n_layers, False)
        assert all(torch.equal(named[k], grads[k]) for k in grads)
        assert torch.equal(fm.from_plan(out_p), dh)
    untiled = eng.FixedPointMap(eng.MeshPlan(r.md, tile_target=-1), r.w, fm.h0, r.md.prb_data, r.nrm)
    assert not untiled.plan.tiled
    g_u, dh_u, dinit_u = untiled.param_vjp_init(H, W)
    r.check_params("param_vjp untiled", g_u, want, want32, TAU["pgrad"])
    r.check("param_vjp untiled dh", dh_u, want_h, want32_h, TAU["pgrad_h"])
    r.check("param_vjp untiled dh_init", dinit_u, want_init, want32_init, TAU["pgrad_h"])
    del want, want_h, want_init, want32, want32_h, want32_init
    _probe_param_vjp(r, fm, r.perm, "param_vjp")
    _probe_param_vjp(r, untiled, np.arange(r.N), "param_vjp untiled")


def test_residual_backward_at_1m(scale):
    """Backward of the residual loss through k_residual_t (A^T r) at 1 000 519 nodes, tile by tile."""
    r = scale(1000519, False)
    u = torch.randn(r.N, 1, generator=torch.Generator().manual_seed(4))
    want = []
    for dt, m in ((torch.float64, r.m64), (torch.float32, r.m)):
        uc = u.to(dt, copy=True).requires_grad_()
        orc.residual_loss(uc, m).backward()
        want.append(uc.grad)
    ud = r.dev_(u).detach().requires_grad_()
    res = r.eng.residual_autograd(r.plan, ud, r.md.y, r.md.a_ij)
    torch.mean(res ** 2).backward()
    r.check("residual backward", ud.grad, want[0], want[1], TAU["residual"])


@pytest.mark.parametrize("mixed", FAMILIES, ids=FAMILY_IDS)
def test_vjp_backward_at_270k(mixed, scale):
    """Backward of the VJP at 270 901 nodes: 2N = 541 802 records (npw = 136; every wave of the last block holds records),
    written in the caller's order, node n at n and N + n; the seam N - 1 | N falls inside a wave and is probed."""
    r = scale(270901, mixed)
    H, V, G = r.dev_(r.h), r.dev_(r.v), r.dev_(r.gb)
    want, want_h, _ = orc.function_vjp_backward(r.s64, r.h.double(), r.h0.double(), r.m64, r.v.double(), r.gb.double())
    want32, want32_h, _ = orc.function_vjp_backward(r.sd, r.h, r.h0, r.m, r.v, r.gb)
    g, dh = r.fm.vjp_backward(H, V, G)
    assert set(g) == set(want)
    r.check_params("vjp_backward", g, want, want32, TAU["jr"])
    r.check("vjp_backward dh", dh, want_h, want32_h, TAU["jr_h"])
    del want, want_h, want32, want32_h
    for name, pos in pr.probes(2 * r.N, seam=r.N).items():
        S = r.support(pr.nodes_at(pos, np.arange(r.N), r.N))
        keep, m32, m64 = r.sub(S, 2)
        v = _masked(r.v, torch.from_numpy(S))
        h, h0, vk, gk = r.h[keep], r.h0[keep], v[keep], r.gb[keep]
        want, want_h, _ = orc.function_vjp_backward(r.s64, h.double(), h0.double(), m64, vk.double(), gk.double())
        want32, want32_h, _ = orc.function_vjp_backward(r.sd, h, h0, m32, vk, gk)
        g, dh = r.fm.vjp_backward(H, r.dev_(v), G)
        _nonzero(f"{r.name} vjp_backward probe [{name}]", want)
        r.check_params(f"vjp_backward probe [{name}]", g, want, want32, TAU["jr"])
        r.check_vec(f"vjp_backward probe [{name}] dh", dh, r.scatter(keep, want_h), r.scatter(keep, want32_h), TAU["jr_h"])


def test_two_layer_param_vjp_at_270k(scale):
    """Two-layer dirichlet block at 270 901 nodes: k_pgrad_reduce_acc adds the layers into one gradient, alpha accumulates
    across them.  The random weights of _random_two_layer put some pre-activations of the 270k-node graph within fp32
    round-off of a ReLU kink, where a state-shaped derivative jumps at one node (measured: one tile of the two-layer JVP at
    1.3e-3 against fp64): dh and dh_init are compared over the whole vector here, the gradients tensor by tensor."""
    r = scale(270901, False)
    sd = _random_two_layer()
    s64 = {k: v.double() for k, v in sd.items()}
    fm = r.eng.FixedPointMap(r.plan, r.eng.PackedWeights(sd, r.dev), r.dev_(r.h0), r.md.prb_data)
    H, W = r.dev_(r.h), r.dev_(r.wv)
    want, want_h, want_init = orc.function_param_vjp(s64, r.h.double(), r.h0.double(), r.m64, r.wv.double())
    want32, want32_h, want32_init = orc.function_param_vjp(sd, r.h, r.h0, r.m, r.wv)
    want, want32 = _filled(want, s64), _filled(want32, sd)
    grads, dh, dinit = fm.param_vjp_init(H, W)
    assert set(grads) == set(want)
    r.check_params("param_vjp L2", grads, want, want32, TAU["pgrad"])
    r.check_vec("param_vjp L2 dh", dh, want_h, want32_h, TAU["pgrad_h"])
    r.check_vec("param_vjp L2 dh_init", dinit, want_init, want32_init, TAU["pgrad_h"])
    flat, out_p = fm.param_vjp_p(fm.to_plan(H), fm.to_plan(W))
    named = r.eng.unpack_param_grads(flat, 2, False)
    assert all(torch.equal(named[k], grads[k]) for k in grads)
    assert torch.equal(fm.from_plan(out_p), dh)


def _dsgps_weights(mixed):
    wd = np.load(os.path.join(GOLDEN, "weights_dsgps_mixed.npz" if mixed else "weights_dsgps.npz"))
    return {n: torch.from_numpy(wd[n]) for n in wd.files if n != "k"}


def _dsgps_grads(sd, names, h, h0, m, w):
    pp = {k: (v.clone().requires_grad_(True) if k in names else v) for k, v in sd.items()}
    hh = h.clone().requires_grad_(True)
    g = torch.autograd.grad(orc.dsgps_step(pp, hh, h0, m), [pp[k] for k in names] + [hh], w, allow_unused=True)
    return {k: (torch.zeros_like(pp[k]) if t is None else t) for k, t in zip(names, g[:-1])}, g[-1]


@pytest.mark.parametrize("mixed", FAMILIES, ids=FAMILY_IDS)
def test_dsgps_step_backward_at_270k(mixed, scale):
    """DS-GPS update and its backward at 270 901 nodes (per-wave partials: TabG, TabGX), dense as on the plan-limit graphs,
    then the probes (gather records, caller's order)."""
    r = scale(270901, mixed)
    _dsgps_products(r)
    eng = r.eng
    sd = _dsgps_weights(mixed)
    s64 = {k: v.double() for k, v in sd.items()}
    names = [k for k in sd if not k.startswith(("autoencoder", "laynorm"))]
    wf, wg = eng.pack_dsgps_train(sd, r.dev)
    H = r.dev_(r.h)
    for name, pos in pr.probes(r.N).items():
        S = r.support(pr.nodes_at(pos, np.arange(r.N), r.N))
        keep, m32, m64 = r.sub(S, 1)
        wv = _masked(r.wv, torch.from_numpy(S))
        h, h0, w = r.h[keep], r.h0[keep], wv[keep]
        want, want_h = _dsgps_grads(s64, names, h.double(), h0.double(), m64, w.double())
        want32, want32_h = _dsgps_grads(sd, names, h, h0, m32, w)
        g, dh = eng.dsgps_step_backward(r.plan, wf, wg, H, r.md.prb_data, r.dev_(wv), r.nrm)
        _nonzero(f"{r.name} dsgps_step_backward probe [{name}]", want)
        r.check_params(f"dsgps_step_backward probe [{name}]", g, want, want32, TAU["dsgps_bw"])
        r.check_vec(f"dsgps_step_backward probe [{name}] dh", dh, r.scatter(keep, want_h), r.scatter(keep, want32_h),
                    TAU["dsgps_bw"])


class _DssBatch:
    pass


def test_dss_step_backward_at_270k(scale):
    """DSS update t = 3 backward at 270 901 nodes (per-block partials, TabF) on the plan of the self-loop-free DSS view."""
    r = scale(270901, False)
    eng = r.eng
    w = np.load(os.path.join(GOLDEN, "weights_dss.npz"))
    sd = {n: torch.from_numpy(w[n]) for n in w.files if n not in ("k", "alpha")}
    t, alpha = 3, 1.0
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
    assert plan.tiled
    names = [n for n in sd if n.startswith((f"phi_to_list.{t}.", f"phi_from_list.{t}.", f"psi_list.{t}."))]
    b64, b32 = _DssBatch(), _DssBatch()
    for b, dt in ((b64, torch.float64), (b32, torch.float32)):
        b.edge_index, b.a_ij_norm, b.b_prime_norm = ei, a_norm.to(dt), bpn.to(dt)

    def grads(p_sd, b, hh, wv):
        pp = {n: (v.clone().requires_grad_(True) if n in names else v) for n, v in p_sd.items()}
        hq = hh.clone().requires_grad_(True)
        g = torch.autograd.grad(orc.dss_step(pp, t, hq, b, alpha), [pp[n] for n in names] + [hq], wv)
        return dict(zip(names, g[:-1])), g[-1]
    want, want_h = grads({n: v.double() for n, v in sd.items()}, b64, r.h.double(), r.wv.double())
    want32, want32_h = grads(sd, b32, r.h, r.wv)
    g, dh = eng.dss_step_backward(plan, eng.pack_dss_train(sd, t, r.dev), t, alpha, r.dev_(r.h), r.dev_(bpn), r.dev_(r.wv))
    r.check_params("dss_step_backward", g, want, want32, TAU["dss_pgrad"])
    r.check("dss_step_backward dh", dh, want_h, want32_h, TAU["dss_bw"], plan.export("perm"), plan.export("tile_ptr"))


# ------------------------------------------------------------------------------------------------ MLP backward
MLP_LENGTHS = [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 262144, 262145, 1000519, 4194305]


def _mlp_ref(x, gy, w1, b1, w2, b2, dt):
    leaves = [t.to(dt).requires_grad_() for t in (x, w1, b1, w2, b2)]
    y = torch.relu(leaves[0] @ leaves[1].t() + leaves[2]) @ leaves[3].t() + leaves[4]
    return torch.autograd.grad(y, leaves, gy.to(dt))


def _row_block_errors(got, want, rows=256):
    """tile_errors over consecutive blocks of ``rows`` rows (the blocks of k_mlp2_bwd), vectorised."""
    g, w = got.detach().cpu().double(), want.double()
    n = g.shape[0]
    pad = (-n) % rows
    d = torch.nn.functional.pad(g - w, (0, 0, 0, pad)).reshape(-1, rows * g.shape[1]).norm(dim=1)
    wb = torch.nn.functional.pad(w, (0, 0, 0, pad)).reshape(-1, rows * w.shape[1]).norm(dim=1)
    nb = torch.full_like(wb, rows)
    nb[-1] = rows - pad
    return d / torch.maximum(wb, 1e-3 * w.norm() * torch.sqrt(nb / n))


@pytest.mark.parametrize("dims", [(1, 10, 10), (10, 10, 1), (3, 7, 5)])
def test_mlp2_backward_at_ragged_lengths(dims, dev):
    """mlp2_autograd / mlp2_backward (TabM, per-block partials) at lengths around 64, 256 and the npw > 64 regime: weight
    gradients per tensor, gx per 256-row block, then the probes.  Rows with a pre-activation within 1e-4 of a ReLU kink
    get no cotangent, so the fp32 kernel and the fp64 reference take the same branch everywhere."""
    eng = pkg("engine")
    din, hid, dout = dims
    gen = torch.Generator().manual_seed(3)
    w1, b1 = torch.randn(hid, din, generator=gen), torch.randn(hid, generator=gen)
    w2, b2 = torch.randn(dout, hid, generator=gen), torch.randn(dout, generator=gen)
    wd = [t.to(dev) for t in (w1, b1, w2, b2)]
    keys = ("w1", "b1", "w2", "b2")
    worst = {}
    for n in MLP_LENGTHS:
        x = torch.randn(n, din, generator=gen)
        gy = torch.randn(n, dout, generator=gen)
        kink = ((x.double() @ w1.double().t() + b1.double()).abs() < 1e-4).any(1)
        gy[kink] = 0
        want = _mlp_ref(x, gy, w1, b1, w2, b2, torch.float64)
        want32 = _mlp_ref(x, gy, w1, b1, w2, b2, torch.float32)
        dl = [r.requires_grad_() for r in [x.to(dev)] + [t.clone() for t in wd]]
        got = torch.autograd.grad(eng.mlp2_autograd(*dl), dl, gy.to(dev))
        what = f"mlp2_backward {dims} n={n}"
        worst[what] = lg.check_params(dict(zip(keys, got[1:])), dict(zip(keys, want[1:])), dict(zip(keys, want32[1:])),
                                      TAU["mlp"], what)
        e, e32 = _row_block_errors(got[0], want[0]), _row_block_errors(want32[0], want[0])
        bad = torch.nonzero(~(e <= torch.clamp(16 * e32, min=TAU["mlp"]))).reshape(-1)
        assert bad.numel() == 0, (what, "gx", {int(b): (float(e[b]), float(e32[b])) for b in bad[:8]})
        k = int(torch.argmax(e))
        worst[what + " gx"] = (float(e[k]), float(e32[k]))
        xd = dl[0].detach()
        for name, pos in pr.probes(n).items():
            rows = torch.from_numpy(pos)
            gp = _masked(gy, rows)
            pw = _mlp_ref(x[rows], gp[rows], w1, b1, w2, b2, torch.float64)
            pw32 = _mlp_ref(x[rows], gp[rows], w1, b1, w2, b2, torch.float32)
            gx, *gw = eng.mlp2_backward(xd, gp.to(dev), *wd[:3])
            pwhat = f"{what} probe [{name}]"
            worst[pwhat] = lg.check_params(dict(zip(keys, gw)), dict(zip(keys, pw[1:])), dict(zip(keys, pw32[1:])),
                                           TAU["mlp"], pwhat)
            full = torch.zeros(n, din, dtype=torch.float64)
            full[rows] = pw[0]
            ex = float((gx.cpu().double() - full).norm()) / max(float(full.norm()), 1e-300)
            ex32 = float((pw32[0].double() - pw[0]).norm()) / max(float(pw[0].norm()), 1e-300)
            assert ex <= max(TAU["mlp"], 16 * ex32), (pwhat, "gx", ex, ex32)
    k = max(worst, key=lambda q: worst[q][0])
    _report(f"mlp2_backward {dims} (worst of {len(worst)}: {k})", *worst[k])
