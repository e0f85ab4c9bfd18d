"""GPU: the float64 backward of the VJP on the device (``psignn_f64_vjp_backward``; ``engine.FixedPointMap64.vjp_backward``,
``engine.jac_loss_grad64``) against autograd's double backward on the CPU oracle in float64 (``orc.function_vjp_backward``), its exact
identities, and the fp32 routes against this new truth.

Where the gates come from.  The rule is that of tests/test_gpu_f64.py, test_gpu_f64_deriv.py and test_gpu_f64_pgrad.py: at most
250 x the float64 oracle's own spread when its summation order changes, per tensor as relative L2.  The oracle was run on every case
of this file (tests/vjp_backward_cases.py) with its edge list permuted and with its nodes renumbered, three seeds each
(scripts/calib_f64_vjp_backward.py, CPU, V = randn(31), Gbar = randn(37); worst tensor in brackets):

====================================  =========  ==================================  ========  ========
case                                  matrices   vectors / scalars                   dH        J^T V
====================================  =========  ==================================  ========  ========
hex13_dirichlet_s0 at h0              1.5e-15    3.6e-15 (alpha.0.weight)            4.8e-16   2.3e-16
hex13_dirichlet_s0 at fp64_result     1.3e-15    2.1e-14 (alpha.0.weight)            5.5e-16   2.7e-16
hex13_mixed_s1 at h0                  1.3e-15    5.3e-15 (alpha.0.weight)            8.3e-16   3.3e-16
hex13_mixed_s1 at fp64_result         1.5e-15    8.1e-15 (alpha.0.weight)            1.2e-15   4.3e-16
original_dirichlet_s0 at h0           1.6e-15    1.6e-14 (alpha.0.bias)              5.6e-16   2.4e-16
original_dirichlet_s0 at fp64_result  1.3e-15    3.1e-15 (alpha.0.weight)            5.6e-16   2.7e-16
slots255_split dirichlet / mixed      7.9e-16 / 2.1e-15  8.6e-16 / 8.5e-15 (alpha.0.bias)  1.5 / 6.5e-16  1.0 / 1.8e-16
ragged65 dirichlet / mixed            8.7e-16 / 4.1e-15  2.2e-14 (alpha.0.bias) / 1.1e-14  6.6e-16 / 2.8e-15  3.2 / 9.8e-16
slots256 dirichlet / mixed            8.5e-16 / 1.3e-15  1.2e-15 / 1.4e-15           2.7 / 8.5e-16  2.1 / 3.7e-16
two layers dirichlet / mixed          1.7 / 1.8e-15  3.8e-15 / 3.5e-15               1.3e-15 / 6.8e-16  5.8 / 3.7e-16
hex60 dirichlet dense / probe         1.5e-15 / 9.6e-16  1.9 / 1.8e-14 (alpha.0.bias)  5.2 / 5.0e-16  2.4 / 3.5e-16
hex60 mixed dense / probe             1.3 / 1.2e-15  1.2e-14 / 5.6e-15 (phi_to b1)   6.3 / 6.1e-16  3.0 / 3.9e-16
line 127 / 128 / 129, both families   <= 7.8e-16  <= 7.6e-16                         0         0
line 1                                not permuted: one self loop, nothing to reorder
====================================  =========  ==================================  ========  ========

* matrices (2-D tensors of more than one row): 250 x 4.1e-15 = 1.0e-12.
* vectors and scalars (biases, laynorm, the one-row gate weight): 250 x 2.2e-14 = 5.5e-12.  The second-order sums cancel less badly
  than the first-order ones of test_gpu_f64_pgrad.py (1.3e-13 there): the regulariser's gradient has no ReLU-only terms to cancel.
* dH: 250 x 2.8e-15 = 7.0e-13, its own gate.
* J^T V is bit-equal to ``fmap.vjp`` and within the gates of tests/test_gpu_f64_deriv.py, (1e-13, 1e-12) and on the structure limits
  (2.7e-13, 1.4e-12).
* identities on hex60 (test 2), the oracle's own defect on the same inputs (a = randn(41), b = randn(43)), dirichlet / mixed:
  symmetry |<a, dH(b)> - <b, dH(a)>| / (|a| |dH(b)|) 6.7e-19 / 4.7e-18; linearity in Gbar, parameters 3.1e-14 / 1.6e-15, dH
  5.5e-16 / 5.9e-16.  Gates 250 x the larger: 1.2e-15, 7.8e-12, 1.5e-13.
* fp32 against the new truth (test 4): the rule and gates tests/test_gpu_gradients_at_scale.py uses for the same quantity against the
  oracle, ``TAU["jr"] = TAU["jr_h"] = 2e-4`` through ``limit_graphs.check_params`` / ``check_tiles``, the float32 oracle's own error
  as e32.
Measured on an MI355X with these gates (worst case over the file): matrices 1.6e-14 (hex60 mixed dense, phi_from W1), vectors 3.1e-14
(hex13_dirichlet_s0 at fp64_result, alpha.0.weight), dH 2.5e-15 (ragged65 mixed); identities 1.3e-19 / 1.9e-18, 4.9e-14 / 2.0e-15,
6.6e-16 / 7.8e-16.
A ReLU mask differing between device and oracle would need a float64 pre-activation within ~1e-15 of zero; with ~1e6 of them that
has probability ~1e-8, so no case is left out and no cap is used.
"""
import numpy as np
import pytest
import torch

import limit_graphs as lg
import vjp_backward_cases as vb
from conftest import pkg, rel_l2
from oracle import psignn_oracle as orc
from test_gpu_f64 import Problem, float64_default
from test_gpu_f64_deriv import GATE, GATE_LIMITS
from test_gpu_gradients_at_scale import TAU

pytestmark = pytest.mark.gpu

GATE_MATRIX = 250 * 4.1e-15
GATE_VECTOR = 250 * 2.2e-14
GATE_DH = 250 * 2.8e-15
GATE_SYM, GATE_LIN_P, GATE_LIN_H = 250 * 4.7e-18, 250 * 3.1e-14, 250 * 5.9e-16

_problems = {}


def _problem(name, dev):
    """The case and its device side, made once: cases that share a mesh and a state dict (hex60 dense / probe, a fixture at its two
    states) share the handles."""
    with float64_default():
        c = vb.make(name)
    key = name.replace("-probe", "").replace("-dense", "").split("@")[0]
    if key not in _problems:
        p = Problem(c.mesh, c.sd, dev, tile_target=c.tile_target, h0=c.h0)
        if c.tiled is not None:
            assert p.plan.tiled == c.tiled, (name, p.plan.tiled)
        _problems[key] = p
    return c, _problems[key]


def _check_grads(got, want, what):
    """Every named tensor within its gate; where the oracle's tensor is all zeros (autograd's None) the device's is too."""
    assert set(got) == set(want), (what, set(got) ^ set(want))
    bad = {}
    for k, t in want.items():
        g = got[k]
        assert g.dtype == torch.float64 and g.shape == t.shape, (what, k, g.dtype, g.shape, t.shape)
        if not bool(t.any()):
            assert not bool(g.any()), (what, k, "the oracle leaves zeros, the device must leave exact zeros")
            continue
        matrix = t.dim() == 2 and t.shape[0] > 1
        r = vb._rel(g, t)
        print(f"F64JR {what} {k}: rel L2 {r:.2e} ({'matrix' if matrix else 'vector'})")
        if not r <= (GATE_MATRIX if matrix else GATE_VECTOR):
            bad[k] = r
    assert not bad, (what, bad)


def _check_case(c, p, V=None, Gbar=None, what=None):
    """vjp_backward of problem p at (H, V, Gbar) against the oracle; returns the device's outputs."""
    what = what or c.name
    V, Gbar = c.V if V is None else V, c.Gbar if Gbar is None else Gbar
    with float64_default():
        want, want_dh, want_jtv = vb.oracle(c, V, Gbar)
    Hd, Vd, Gd = c.H.to(p.dev), V.to(p.dev), Gbar.to(p.dev)
    grads, dh, jtv = p.fmap.vjp_backward(Hd, Vd, Gd)
    assert dh.dtype == jtv.dtype == torch.float64 and dh.shape == jtv.shape == c.H.shape
    _check_grads(grads, want, what)
    r = vb._rel(dh, want_dh)
    print(f"F64JR {what} dH: rel L2 {r:.2e}")
    assert r <= GATE_DH, (what, "dH", r)
    zero = want_dh == 0   # rows no probe reaches: exact zeros on the device too
    assert not bool(dh.cpu()[zero].any()), (what, "dH is not exactly zero where the oracle's is")
    gate = GATE_LIMITS if c.limits else GATE
    rj, mx = rel_l2(jtv.cpu(), want_jtv), float((jtv.cpu() - want_jtv).abs().max())
    print(f"F64JR {what} J^T V: rel L2 {rj:.2e} max-abs {mx:.2e}")
    assert rj <= gate[0] and mx <= gate[1], (what, "J^T V", rj, mx)
    assert torch.equal(jtv, p.fmap.vjp(Hd, Vd)), what
    return grads, dh, jtv


def _same_bits(a, b):
    return set(a[0]) == set(b[0]) and all(torch.equal(a[0][k], b[0][k]) for k in a[0]) and torch.equal(a[1], b[1]) and torch.equal(
        a[2], b[2])


# ----------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("name", vb.NAMES)
def test_against_the_float64_oracle(name, dev):
    c, p = _problem(name, dev)
    first = _check_case(c, p)
    Hd, Vd, Gd = c.H.to(dev), c.V.to(dev), c.Gbar.to(dev)
    assert _same_bits(first, p.fmap.vjp_backward(Hd, Vd, Gd))   # fixed summation order: the same call gives the same bits
    if name.startswith("two_layers"):
        layer0 = [k for k in first[0] if "_list.0." in k]
        assert len(layer0) == 12
        if p.w.mixed:   # only the last iteration reaches the output
            assert all(not bool(first[0][k].any()) for k in layer0)
        else:
            assert all(bool(first[0][k].any()) for k in layer0)
    if name.startswith("hex60"):
        chunk = int(pkg("_native").lib().psignn_f64_param_vjp_chunk_rows())
        assert chunk == vb.CHUNK and -(-p.plan.N // chunk) > 64 and p.plan.N % chunk != 0   # both fold stages, a ragged tail
    if name.endswith("@h0"):   # float32 inputs are widened exactly
        assert _same_bits(p.fmap.vjp_backward(Hd.float(), Vd.float(), Gd.float()),
                          p.fmap.vjp_backward(Hd.float().double(), Vd.float().double(), Gd.float().double()))


# ----------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("mixed", [False, True])
def test_exact_identities_on_hex60(mixed, dev):
    """No oracle: the Hessian of phi = <V, f(H)> is symmetric, so <a, dH(V, Gbar = b)> = <b, dH(V, Gbar = a)>; everything is linear
    in Gbar; and the same call gives the same bits.  The gates are 250 x the defect the CPU oracle leaves in the same identities on
    the same inputs (module docstring)."""
    c, p = _problem(f"hex60-{'mixed' if mixed else 'dirichlet'}-dense", dev)
    Hd, Vd = c.H.to(dev), c.V.to(dev)
    a, b = vb.randn(c.H.shape, 41).to(dev), vb.randn(c.H.shape, 43).to(dev)
    sym, lin_p, lin_h = vb.identity_defects(lambda G: p.fmap.vjp_backward(Hd, Vd, G), a, b)
    print(f"F64JR {c.name} identities: symmetry {sym:.2e} linearity parameters {lin_p:.2e} dH {lin_h:.2e}")
    assert sym <= GATE_SYM and lin_p <= GATE_LIN_P and lin_h <= GATE_LIN_H, (sym, lin_p, lin_h)
    assert _same_bits(p.fmap.vjp_backward(Hd, Vd, a), p.fmap.vjp_backward(Hd, Vd, a))


# ----------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("name", ["hex13_dirichlet_s0", "hex13_mixed_s1"])
def test_jac_loss_grad64(name, dev):
    """Two fixed probes at the stored float64 fixed point, against ``function_vjp_backward`` summed over the probes with
    Gbar_i = 2 J^T v_i / (n N d) -- the regulariser part of ``orc.training_step(..., jac_weight=1, probe=...)``."""
    c, p = _problem(f"{name}@fp64_result", dev)
    eng = p.eng
    probes = [vb.randn(c.H.shape, 51), vb.randn(c.H.shape, 52)]
    out = eng.jac_loss_grad64(p.md, p.sd, c.H.to(dev), [v.to(dev) for v in probes])
    assert set(out) == {"jac_loss", "grads", "dh", "jtv"} and out["jtv"].shape == (2,) + tuple(c.H.shape)
    scale = 1.0 / (2 * c.H.numel())
    want_loss, want, want_dh = 0.0, None, None
    for i, v in enumerate(probes):
        with float64_default():
            _, _, jtv = vb.oracle(c, v, torch.zeros_like(v))
            g, dh, _ = vb.oracle(c, v, 2 * scale * jtv)
        want_loss += float((jtv * jtv).sum()) * scale
        want = g if want is None else {k: want[k] + g[k] for k in g}
        want_dh = dh if want_dh is None else want_dh + dh
        assert vb._rel(out["jtv"][i], jtv) <= GATE[0]
    print(f"F64JR {name} jac_loss {out['jac_loss']:.12e} (oracle {want_loss:.12e})")
    assert abs(out["jac_loss"] - want_loss) <= GATE[0] * want_loss
    assert all(k.startswith("deqdss.f.") for k in out["grads"])
    _check_grads({k[len("deqdss.f."):]: t for k, t in out["grads"].items()}, want, f"{name} jac_loss_grad64")
    r = vb._rel(out["dh"], want_dh)
    print(f"F64JR {name} jac_loss_grad64 dH: rel L2 {r:.2e}")
    assert r <= GATE_DH, (name, r)
    # the hand composition, bit for bit
    Hd = c.H.to(dev)
    g0, d0, j0 = p.fmap.vjp_backward(Hd, probes[0].to(dev), 2 * scale * p.fmap.vjp(Hd, probes[0].to(dev)))
    g1, d1, j1 = p.fmap.vjp_backward(Hd, probes[1].to(dev), 2 * scale * p.fmap.vjp(Hd, probes[1].to(dev)))
    assert torch.equal(out["dh"], d0 + d1) and torch.equal(out["jtv"], torch.stack([j0, j1]))
    assert all(torch.equal(out["grads"]["deqdss.f." + k], g0[k] + g1[k]) for k in g0)


# ----------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("name", ["hex13_dirichlet_s0@h0", "hex13_mixed_s1@h0", "hex60-dirichlet-dense", "hex60-mixed-dense"])
def test_fp32_routes_against_the_float64_device(name, dev):
    """``FixedPointMap.vjp_backward`` (fp32: the gather route and, where it applies, the tile route) against
    ``FixedPointMap64.vjp_backward`` at the state two f steps from h0, by the rule of tests/test_gpu_gradients_at_scale.py."""
    c, p = _problem(name, dev)
    eng, N = p.eng, p.plan.N
    h0_32 = p.h0.float().to(dev)
    plan32 = eng.MeshPlan(p.md)
    fm32 = eng.FixedPointMap(plan32, eng.PackedWeights(p.sd, dev), h0_32, p.md.prb_data, getattr(p.md, "unit_normal_vector", None))
    H = fm32(fm32(h0_32)).contiguous()
    gen = torch.Generator().manual_seed(21)
    V, G = (0.3 * torch.randn(N, 10, generator=gen) for _ in range(2))
    G /= N
    truth, truth_dh, _ = p.fmap.vjp_backward(H, V.to(dev), G.to(dev))
    truth = {k: t.cpu() for k, t in truth.items()}
    want32, want32_dh, _ = orc.function_vjp_backward(p.sd, H.cpu(), p.h0.float(), p.mesh, V, G)   # the float32 oracle: e32
    perm, tile_ptr = np.arange(N), lg.chunk_tiles(N)
    routes = [("gather", False)] + ([("tiled", True)] if fm32.can_tile_vjp_backward() else [])
    if name == "hex60-dirichlet-dense":
        assert len(routes) == 2   # the tile route is part of this case
    for route, tiled in routes:
        got, dh = fm32.vjp_backward(H, V.to(dev), G.to(dev), tiled=tiled)
        e, e32 = lg.check_params(got, truth, want32, TAU["jr"], f"{name} fp32 {route} vjp_backward vs float64 device")
        print(f"F64JR {name} fp32 {route} vs float64 device: parameters worst e {e:.2e} (float32 oracle {e32:.2e})")
        e, e32 = lg.check_tiles(dh, truth_dh.cpu(), want32_dh, perm, tile_ptr, TAU["jr_h"], f"{name} fp32 {route} dH")
        print(f"F64JR {name} fp32 {route} vs float64 device: dH worst tile e {e:.2e} (float32 oracle {e32:.2e})")


# ----------------------------------------------------------------------------------------------------------------- 5
def test_workspace_sizes_and_refusals_on_an_open_handle(dev):
    """The workspace query is the documented formula on real handles (single layer, chain, mixed); aliasing, a layer count out of
    range and a workspace that is too small are error codes, and the message names the bytes."""
    from test_host_f64_vjp_backward import _documented_size
    nat = pkg("_native")
    lib, ptr = nat.lib(), nat.ptr
    chunk = int(lib.psignn_f64_param_vjp_chunk_rows())
    for name in ("hex13_dirichlet_s0@h0", "hex13_mixed_s1@h0", "line129-dirichlet"):
        c, p = _problem(name, dev)
        mixed = p.w.mixed
        for nl in (1, 2, 3):
            want = _documented_size(p.plan.N, nl, mixed, chunk, int(lib.psignn_f64_weights_size(int(mixed), 1)))
            assert lib.psignn_f64_vjp_backward_workspace_doubles(p.fmap.handle, nl) == want > 0, (name, nl)
        assert lib.psignn_f64_vjp_backward_workspace_doubles(p.fmap.handle, 0) == -1
    c, p = _problem("hex13_dirichlet_s0@h0", dev)
    fm, N = p.fmap, p.plan.N
    need = lib.psignn_f64_vjp_backward_workspace_doubles(fm.handle, 1)
    H, v, gb, dh, jtv = (torch.zeros(N, 10, dtype=torch.float64, device=dev) for _ in range(5))
    grad = torch.zeros(lib.psignn_f64_weights_size(0, 1), dtype=torch.float64, device=dev)
    work = torch.zeros(need, dtype=torch.float64, device=dev)
    call = lambda nl, o, j, n: lib.psignn_f64_vjp_backward(fm.handle, ptr(fm.wflat), nl, ptr(H), ptr(fm.h0), ptr(fm.prb), None, ptr(v),
                                                          ptr(gb), ptr(grad), ptr(o), j, ptr(work), n, None)
    assert call(1, H, None, need) < 0 and "alias" in lib.psignn_last_error().decode()
    assert call(1, v, None, need) < 0 and call(1, gb, None, need) < 0
    assert call(1, dh, ptr(dh), need) < 0 and call(1, dh, ptr(H), need) < 0 and call(1, dh, ptr(gb), need) < 0
    assert call(0, dh, None, need) < 0 and call(65, dh, None, need) < 0
    assert call(1, dh, None, need - 1) < 0
    assert f"{need * 8} bytes" in lib.psignn_last_error().decode()
    assert call(1, dh, None, need) == 0 and call(1, dh, ptr(jtv), need) == 0
    torch.cuda.synchronize(dev)
