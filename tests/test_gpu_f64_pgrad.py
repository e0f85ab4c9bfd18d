"""GPU: the float64 parameter gradients on the device (``psignn_f64_param_vjp``, ``psignn_mlp2_f64_backward``;
``engine.FixedPointMap64.param_vjp``, ``mlp2_64_backward``, ``implicit_grad64``) against autograd on the CPU oracle in float64
(``orc.function_param_vjp``), and the fp32 parameter-gradient kernels against this new truth.

Where the gates come from.  The rule is that of tests/test_gpu_f64.py and tests/test_gpu_f64_deriv.py: at most 250 x the float64
oracle's own spread when its summation order changes, applied per tensor as relative L2.  A sum over nodes has two freedoms, so the
oracle was run with its edge list permuted and with its nodes renumbered, three seeds each (scripts/calib_f64_pgrad.py, CPU,
w = randn; worst tensor in brackets):

====================================  ===========  ==============================  ========  ========
graph                                 matrices     vectors / scalars               J^T w     dH_init
====================================  ===========  ==============================  ========  ========
hex13_dirichlet_s0 at h0              4.4e-15      5.6e-14 (alpha.0.bias)          2.3e-16   0
hex13_dirichlet_s0 at fp64_result     2.1e-15      2.3e-14 (alpha.0.bias)          2.7e-16   0
hex13_mixed_s1 at h0                  7.6e-15      1.3e-14 (alpha.0.weight)        3.3e-16   0
hex13_mixed_s1 at fp64_result         6.7e-15      4.4e-15 (phi_to_list.0 b1)      4.3e-16   0
original_dirichlet_s0 at h0           1.6e-15      1.3e-13 (alpha.0.bias)          2.4e-16   0
original_dirichlet_s0 at fp64_result  1.3e-15      3.0e-14 (alpha.0.bias)          2.7e-16   0
slots255_split dirichlet / mixed      1.2 / 1.4e-15  1.5e-15 / 7.8e-16             1.0 / 1.8e-16  0
ragged65 dirichlet / mixed            1.4 / 1.8e-15  6.6e-14 (alpha.0.bias) / 1.8e-15  3.2 / 9.8e-16  0
slots256 dirichlet / mixed            9.9e-16 / 1.0e-15  1.1e-15 / 7.3e-16         2.1 / 3.7e-16  0
two layers dirichlet / mixed          1.7 / 2.1e-15  1.7 / 2.1e-15                 5.8 / 3.7e-16  3.9e-17 / 0
hex60 dirichlet dense / probe         1.5 / 1.0e-15  4.8 / 3.3e-14 (alpha.0.bias)  2.4 / 1.4e-16  0
hex60 mixed dense / probe             1.8e-15 / 3.1e-16  3.1e-15 / 3.1e-15         3.0 / 3.4e-16  0
MLP backward, n in {1, 255, 257, 10 981}  <= 4.2e-15 (all parameter tensors; mixed encoder, n = 10 981), gx: 0 (row-local)
====================================  ===========  ==============================  ========  ========

* matrices (2-D tensors of more than one row): 250 x 7.6e-15 = 1.9e-12.
* vectors and scalars (biases, laynorm, the one-row gate weight): their sums cancel -- alpha.0.bias is sum_n gal_n of either sign --
  and spread 17 x more than the matrices, so they have their own gate: 250 x 1.3e-13 = 3.3e-11.
* J^T w: the gates of tests/test_gpu_f64_deriv.py, (1e-13, 1e-12) and on the structure limits (2.7e-13, 1.4e-12); it is also bit-equal
  to ``fmap.vjp``.  dH_init of a chain holds inner cotangents, which are such products: the same gates; on a single-layer block it is a
  copy, compared bit for bit.
* MLP backward: parameters 250 x 4.2e-15 = 1.05e-12; gx is row-local like the forward MLP: the 1e-13 of tests/test_gpu_f64.py.
* fp32 against the new truth (test 5): the rule and gate tests/test_gpu_gradients_at_scale.py uses for the same quantity against
  the oracle, ``TAU["pgrad"] = 2e-5`` through ``limit_graphs.check_params``, the float32 oracle's own error as e32.
A ReLU mask differing between device and oracle would need a float64 pre-activation within ~1e-15 of zero; with ~1e6 of them that
has probability ~1e-8, so no case is left out and no cap is used.
"""
import pytest
import torch

import limit_graphs as lg
from conftest import load_case, load_weights, pkg, rel_l2
from oracle import psignn_oracle as orc
from test_gpu_f64 import FIXTURES, Problem, _ae, _random_two_layer_mixed, fixture_problem, float64_default
from test_gpu_f64_deriv import GATE, GATE_LIMITS
from test_gpu_plan_limits import _random_two_layer

pytestmark = pytest.mark.gpu

GATE_MATRIX = 250 * 7.6e-15
GATE_VECTOR = 250 * 1.3e-13
GATE_MLP = 250 * 4.2e-15
GATE_MLP_GX = 1e-13
TAU_PGRAD = 2e-5


def _rel(got, want):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    d = float(want.norm())
    return float((got - want).norm()) / d if d > 0 else float((got - want).norm())


def _close(got, want, what, gate=GATE):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    rel, mx = rel_l2(got, want), float((got - want).abs().max())
    print(f"F64P {what}: rel L2 {rel:.2e} max-abs {mx:.2e}")
    assert rel <= gate[0] and mx <= gate[1], (what, rel, mx)


def _check_grads(got, want, what):
    """Every named tensor within its gate; autograd's None entries (allow_unused) are exact zeros on the device."""
    assert set(got) == set(want), (what, set(got) ^ set(want))
    bad = {}
    for k, t in want.items():
        g = got[k]
        assert g.dtype == torch.float64
        if t is None:
            assert not bool(g.any()), (what, k, "autograd leaves None, the device must leave exact zeros")
            continue
        assert g.shape == t.shape, (what, k, g.shape, t.shape)
        matrix = t.dim() == 2 and t.shape[0] > 1
        r = _rel(g, t)
        print(f"F64P {what} {k}: rel L2 {r:.2e} ({'matrix' if matrix else 'vector'})")
        if not r <= (GATE_MATRIX if matrix else GATE_VECTOR):
            bad[k] = r
    assert not bad, (what, bad)


def _oracle(p, H, w):
    with float64_default():
        return orc.function_param_vjp(p.s64, H.clone(), p.h0, p.m64, w)


def _dirichlet_rows(p):
    """The rows the oracle resets to h_initial (function_forward: tags[:, 1] == 1 for mixed, tags == 1 for dirichlet)."""
    t = p.mesh.tags
    rows = torch.zeros(p.mesh.num_nodes, dtype=torch.bool)
    rows[torch.where(t[:, 1] == 1 if p.w.mixed else t == 1)[0]] = True
    return rows


def _param_vjp(p, H, w, what, gate=GATE, single_layer=True):
    """param_vjp of problem p at (H, w) against the oracle; returns the device's outputs."""
    want, want_h, want_init = _oracle(p, H, w)
    Hd, wd = H.to(p.dev), w.to(p.dev)
    grads, dh, dinit = p.fmap.param_vjp(Hd, wd)
    assert dh.dtype == dinit.dtype == torch.float64 and dh.shape == dinit.shape == H.shape
    _check_grads(grads, want, what)
    _close(dh, want_h, f"{what} J^T w", gate)
    assert torch.equal(dh, p.fmap.vjp(Hd, wd)), what
    if single_layer:   # a copy: w on the Dirichlet rows, 0 elsewhere
        expect = torch.where(_dirichlet_rows(p)[:, None], w, torch.zeros_like(w))
        assert torch.equal(dinit.cpu(), expect) and torch.equal(dinit.cpu(), want_init), what
    else:
        _close(dinit, want_init, f"{what} dH_init", gate)
    return grads, dh, dinit


def _same_bits(a, b):
    return set(a[0]) == set(b[0]) and all(torch.equal(a[0][k], b[0][k]) for k in a[0]) and torch.equal(a[1], b[1]) and (
        (a[2] is None and b[2] is None) or torch.equal(a[2], b[2]))


def _w(shape, seed=31):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


# ----------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("name", FIXTURES)
def test_param_vjp_on_the_fixtures(name, dev):
    p = fixture_problem(name, dev)
    for at, H in (("h0", p.h0), ("fp64_result", torch.from_numpy(p.golden["fp64_result"]))):
        w = _w(H.shape)
        first = _param_vjp(p, H, w, f"{name} at {at}")
        Hd, wd = H.to(dev), w.to(dev)
        assert _same_bits(first, p.fmap.param_vjp(Hd, wd))   # fixed summation order: the same call gives the same bits
        # float32 inputs are widened exactly
        assert _same_bits(p.fmap.param_vjp(Hd.float(), wd.float()), p.fmap.param_vjp(Hd.float().double(), wd.float().double()))
        g, dh, none = p.fmap.param_vjp(Hd, wd, with_init=False)
        assert none is None and _same_bits(first[:2] + (None,), (g, dh, None))


# ----------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("case", ["slots255_split", "ragged65", "slots256"])
def test_structure_limits(case, mixed, dev):
    c = lg.build(case, mixed)
    N = c.mesh.num_nodes
    gen = torch.Generator().manual_seed(21)
    H = 0.3 * torch.randn(N, 10, generator=gen, dtype=torch.float64)
    H0 = 0.3 * torch.randn(N, 10, generator=gen, dtype=torch.float64)
    p = Problem(c.mesh, load_weights("mixed" if mixed else "dirichlet"), dev, tile_target=c.tile_target, h0=H0)
    assert p.plan.tiled == c.tiled, (case, p.plan.tiled)
    if case == "slots256":
        assert not p.plan.tiled
    _param_vjp(p, H, _w(H.shape), f"{case}-{'mixed' if mixed else 'dirichlet'}", GATE_LIMITS)


# ----------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("mixed", [False, True])
def test_two_layer_block(mixed, dev):
    """n_layers = 2.  Dirichlet: the chain -- alpha accumulates over both layers, laynorm comes from the last, dH_init sums both layers'
    Dirichlet rows.  Mixed: only the last iteration reaches the output, layer 0's three modules get exact zeros."""
    _, mesh = load_case("hex13_mixed_s1" if mixed else "hex13_dirichlet_s0")
    sd = _random_two_layer_mixed() if mixed else _random_two_layer()
    gen = torch.Generator().manual_seed(22)
    H = 0.3 * torch.randn(mesh.num_nodes, 10, generator=gen, dtype=torch.float64)
    H0 = 0.3 * torch.randn(mesh.num_nodes, 10, generator=gen, dtype=torch.float64)
    p = Problem(mesh, sd, dev, h0=H0)
    assert p.w.n_layers == 2 and p.w.mixed == mixed
    w = _w(H.shape)
    out = _param_vjp(p, H, w, f"two layers {'mixed' if mixed else 'dirichlet'}", single_layer=mixed)
    assert _same_bits(out, p.fmap.param_vjp(H.to(dev), w.to(dev)))
    layer0 = [k for k in out[0] if ("_list.0." in k)]
    assert len(layer0) == 12
    if mixed:
        assert all(not bool(out[0][k].any()) for k in layer0)
    else:
        assert all(bool(out[0][k].any()) for k in layer0)
        rows = _dirichlet_rows(p)
        assert not torch.equal(out[2].cpu()[rows], w[rows])   # more than the last layer's copy
        assert not bool(out[2].cpu()[~rows].any())


# ----------------------------------------------------------------------------------------------------------------- 4
_hex60 = {}


def _hex60_problem(mixed, dev):
    if mixed not in _hex60:
        mesh = pkg("data").make_hex_problem(60, seed=3, mixed=mixed, compute_sol=False)
        assert mesh.num_nodes == 10981
        _hex60[mixed] = Problem(mesh, load_weights("mixed" if mixed else "dirichlet"), dev)
    return _hex60[mixed]


@pytest.mark.parametrize("probe", [False, True])
@pytest.mark.parametrize("mixed", [False, True])
def test_many_chunks_with_a_ragged_tail(mixed, probe, dev):
    """10 981 nodes: 86 chunks of 128 rows (more than one group of the first reduction stage) with a ragged tail.  Dense w, and w
    non-zero only on the rows next to chunk boundaries, where a dropped or doubled partial is an O(1) error in some tensor."""
    p = _hex60_problem(mixed, dev)
    N = p.plan.N
    c = int(pkg("_native").lib().psignn_f64_param_vjp_chunk_rows())
    assert c >= 1 and N > 2 * c and N % c != 0
    w = _w(p.h0.shape)
    if probe:
        rows = [0, c - 1, c, c + 1, 2 * c - 1, 2 * c, N - 1]
        sparse = torch.zeros_like(w)
        sparse[rows] = w[rows]
        w = sparse
    _param_vjp(p, p.h0, w, f"hex60 {'mixed' if mixed else 'dirichlet'} {'probe' if probe else 'dense'}")


# ----------------------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("name", FIXTURES)
def test_fp32_kernels_against_the_float64_device(name, dev):
    """``FixedPointMap.param_vjp_init`` (fp32) against ``FixedPointMap64.param_vjp`` at the state two f steps from h0."""
    p = fixture_problem(name, dev)
    eng = p.eng
    fm32 = eng.FixedPointMap(eng.MeshPlan(p.md), eng.PackedWeights(p.sd, dev), p.h0.float().to(dev), p.md.prb_data,
                             getattr(p.md, "unit_normal_vector", None))
    h0_32 = p.h0.float().to(dev)
    H = fm32(fm32(h0_32)).contiguous()
    w = _w(H.shape).float()
    got, _, _ = fm32.param_vjp_init(H, w.to(dev))
    truth, _, _ = p.fmap.param_vjp(H, w.to(dev))
    want32, _, _ = orc.function_param_vjp(p.sd, H.cpu(), p.h0.float(), p.mesh, w)   # the float32 oracle: its own error is e32
    zero = lambda d, like: {k: (torch.zeros_like(like[k]) if t is None else t) for k, t in d.items()}
    truth = {k: t.cpu() for k, t in truth.items()}
    e, e32 = lg.check_params(got, truth, zero(want32, truth), TAU_PGRAD, f"{name} fp32 param_vjp_init vs float64 device")
    print(f"F64P {name} fp32 vs float64 device: worst e {e:.2e} (float32 oracle {e32:.2e})")


# ----------------------------------------------------------------------------------------------------------------- 6
def _mlp_cases():
    out = []
    for fam in ("dirichlet", "mixed"):
        sd = load_weights(fam)
        out += [(f"{fam} encoder", _ae(sd, "encoder")), (f"{fam} decoder", _ae(sd, "decoder"))]
    gen = torch.Generator().manual_seed(7)
    out.append(("random 16-16-16", [torch.randn(16, 16, generator=gen, dtype=torch.float64) * 0.3,
                                    torch.randn(16, generator=gen, dtype=torch.float64) * 0.1,
                                    torch.randn(16, 16, generator=gen, dtype=torch.float64) * 0.3,
                                    torch.randn(16, generator=gen, dtype=torch.float64) * 0.1]))
    return out


@pytest.mark.parametrize("n", [1, 255, 257, 10981])
def test_mlp2_64_backward(n, dev):
    eng = pkg("engine")
    for name, ws in _mlp_cases():
        ws = [t.double() for t in ws]
        x, gy = _w((n, ws[0].shape[1]), 41), _w((n, ws[2].shape[0]), 42)
        xs = x.clone().requires_grad_(True)
        ps = [t.clone().requires_grad_(True) for t in ws]
        y = torch.nn.functional.linear(torch.relu(torch.nn.functional.linear(xs, ps[0], ps[1])), ps[2], ps[3])
        want = torch.autograd.grad(y, [xs] + ps, gy)
        xd, gd = x.to(dev), gy.to(dev)
        got = eng.mlp2_64_backward(xd, gd, *ws[:3])
        assert len(got) == 5 and all(t.dtype == torch.float64 for t in got)
        r = _rel(got[0], want[0])
        print(f"F64P mlp {name} n {n} gx: rel L2 {r:.2e}")
        assert got[0].shape == x.shape and r <= GATE_MLP_GX, (name, n, r)
        for k, (g, t) in zip(("gW1", "gb1", "gW2", "gb2"), zip(got[1:], want[1:])):
            r = _rel(g, t)
            print(f"F64P mlp {name} n {n} {k}: rel L2 {r:.2e}")
            assert g.shape == t.shape and r <= GATE_MLP, (name, n, k, r)
        again = eng.mlp2_64_backward(xd, gd, *ws[:3])
        assert all(torch.equal(a, b) for a, b in zip(got, again)), (name, n)
        skip = eng.mlp2_64_backward(xd, gd, *ws[:3], need_gx=False)
        assert skip[0] is None and all(torch.equal(a, b) for a, b in zip(got[1:], skip[1:])), (name, n)


# ----------------------------------------------------------------------------------------------------------------- 7
@pytest.mark.parametrize("name", FIXTURES)
def test_implicit_grad64(name, dev):
    p = fixture_problem(name, dev)
    eng = p.eng
    hs = torch.from_numpy(p.golden["fp64_result"]).to(dev)
    grad = _w(hs.shape, 33).to(dev)
    out = eng.implicit_grad64(p.md, p.sd, hs, grad)
    assert set(out) == {"grads", "y", "dh", "adjoint"} and out["adjoint"] is not None
    # the hand composition, bit for bit
    adj = eng.adjoint64(p.md, p.sd, hs, grad)
    y = adj["result"]
    assert torch.equal(out["y"], y)
    enc = _ae(p.sd, "encoder")
    h0 = eng.mlp2_64(p.md.x, *enc)
    fmap = eng.FixedPointMap64(p.plan, p.w, h0, p.md.prb_data, p.md.edge_attr, getattr(p.md, "unit_normal_vector", None))
    named, dh, dinit = fmap.param_vjp(hs, y)
    fmap.close()
    genc = eng.mlp2_64_backward(p.md.x, dinit, *enc[:3], need_gx=False)[1:]
    enc_names = [f"autoencoder.encoder.mlp.mlp.{i}.{q}" for i, q in ((0, "weight"), (0, "bias"), (2, "weight"), (2, "bias"))]
    hand = {"deqdss.f." + k: t for k, t in named.items()}
    hand.update(zip(enc_names, genc))
    assert set(out["grads"]) == set(hand) and all(torch.equal(out["grads"][k], hand[k]) for k in hand)
    assert torch.equal(out["dh"], dh)
    given = eng.implicit_grad64(p.md, p.sd, hs, grad, y=y)
    assert given["adjoint"] is None and torch.equal(given["y"], y) and torch.equal(given["dh"], dh)
    assert all(torch.equal(given["grads"][k], hand[k]) for k in hand)
    # against the oracle at the device's own y: f's parameters, then encoder autograd on dH_init
    want, _, want_init = _oracle(p, hs.cpu(), y.cpu())
    _check_grads({k[len("deqdss.f."):]: t for k, t in out["grads"].items() if k.startswith("deqdss.f.")}, want, f"{name} implicit")
    with float64_default():
        ps = [p.s64[k].clone().requires_grad_(True) for k in enc_names]
        h0c = torch.nn.functional.linear(torch.relu(torch.nn.functional.linear(p.m64.x, ps[0], ps[1])), ps[2], ps[3])
        want_enc = torch.autograd.grad(h0c, ps, want_init)
    for k, t in zip(enc_names, want_enc):
        r = _rel(out["grads"][k], t)
        print(f"F64P {name} implicit {k}: rel L2 {r:.2e}")
        assert r <= GATE_MLP, (name, k, r)


# ----------------------------------------------------------------------------------------------------------------- 8
def test_refusals_on_an_open_handle(dev):
    """Aliasing, a layer count out of range and a workspace that is too small are error codes; the message names the bytes."""
    nat = pkg("_native")
    p = fixture_problem("hex13_dirichlet_s0", dev)
    fm, lib = p.fmap, nat.lib()
    N = p.plan.N
    c = lib.psignn_f64_param_vjp_chunk_rows()
    need = lib.psignn_f64_param_vjp_workspace_doubles(fm.handle, 1)
    assert need == 3 * N * 10 + -(-N // c) * lib.psignn_f64_weights_size(0, 1)
    assert lib.psignn_f64_param_vjp_workspace_doubles(fm.handle, 3) == (3 + 2 + 2) * N * 10 + -(-N // c) * lib.psignn_f64_weights_size(0, 1)
    assert lib.psignn_f64_param_vjp_workspace_doubles(fm.handle, 0) == -1
    H, x, out, init = (torch.zeros(N, 10, dtype=torch.float64, device=dev) for _ in range(4))
    grad = torch.zeros(lib.psignn_f64_weights_size(0, 1), dtype=torch.float64, device=dev)
    work = torch.zeros(need, dtype=torch.float64, device=dev)
    ptr = nat.ptr
    call = lambda nl, h, w, o, i, n: lib.psignn_f64_param_vjp(fm.handle, ptr(fm.wflat), nl, ptr(h), ptr(fm.h0), ptr(fm.prb), None,
                                                              ptr(w), ptr(grad), ptr(o), i, ptr(work), n, None)
    assert call(1, H, x, H, None, need) < 0 and "alias" in lib.psignn_last_error().decode()
    assert call(1, H, x, x, None, need) < 0 and call(1, H, x, out, ptr(out), need) < 0 and call(1, H, x, out, ptr(H), need) < 0
    assert call(0, H, x, out, None, need) < 0 and call(65, H, x, out, None, need) < 0
    assert call(1, H, x, out, None, need - 1) < 0
    assert f"{need * 8} bytes" in lib.psignn_last_error().decode()
    assert call(1, H, x, out, ptr(init), need) == 0
    # the MLP backward: a short workspace names its bytes too
    xs, gy = torch.zeros(300, 4, dtype=torch.float64, device=dev), torch.zeros(300, 10, dtype=torch.float64, device=dev)
    w1, b1, w2 = (torch.zeros(s, dtype=torch.float64, device=dev) for s in ((10, 4), (10,), (10, 10)))
    nw = lib.psignn_mlp2_f64_backward_workspace_doubles(300, 4, 10, 10)
    assert nw == 3 * (40 + 10 + 100 + 10)
    gflat, mwork = torch.zeros(160, dtype=torch.float64, device=dev), torch.zeros(nw, dtype=torch.float64, device=dev)
    mlp = lambda n: lib.psignn_mlp2_f64_backward(ptr(xs), ptr(gy), 300, 4, 10, 10, ptr(w1), ptr(b1), ptr(w2), None, ptr(gflat),
                                                 ptr(mwork), n, None)
    assert mlp(nw - 1) < 0 and f"{nw * 8} bytes" in lib.psignn_last_error().decode()
    assert mlp(nw) == 0
    torch.cuda.synchronize(dev)
