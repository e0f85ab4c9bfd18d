"""GPU: the float64 losses and the one-call float64 training step on the device (``psignn_residual_f64``, ``psignn_residual_t_f64``,
``psignn_mse_f64``; ``engine.residual64``, ``residual64_t``, ``mse64``, ``train_step64``) against the CPU oracle in float64
(``orc.training_step`` and its restatement at a given state, tests/train_step_ref.py), and the fp32 training step against this new
truth.

Where the gates come from.  The rule is that of tests/test_gpu_f64_pgrad.py: at most 250 x the float64 oracle's own spread when its
summation order changes, as relative L2.  scripts/calib_f64_train_step.py ran the oracle's forms on every case of this file with the
edge list permuted and with the nodes renumbered, three seeds each (CPU; worst tensor in brackets):

=====================================  ================================================================================
residual, worst over the 16 graphs     A u - y 3.6e-16 (slots256 dirichlet), A^T w 5.1e-16 (slots256 mixed); off the structure
                                       limits 1.1e-16 / 1.3e-16; the oracle's own defect in <w, A u> = <A^T w, u> 2.1e-16 (line1)
mean((a - b)^2), elements permuted     n = 1: 0; 1023: 6.8e-16; 1024: 1.1e-15; 1025: 6.6e-16; 262 145: 6.2e-15; 109 810: 1.3e-14
=====================================  ================================================================================

``train_step_ref`` at the oracle step's own h* and y (bit-equal to ``orc.training_step`` in all five cases), reordered:

======================  =========  ========================  ==============================  ========  ===========================
case                    matrices   vectors / scalars of f    autoencoder tensors             grad_h    loss scalars
======================  =========  ========================  ==============================  ========  ===========================
hex13_dirichlet_s0      6.9e-16    6.1e-15 (alpha.0.bias)    3.2e-13 (decoder 0.weight)      1.0e-12   3.8e-14 (residual_loss)
hex13_mixed_s1          4.4e-16    7.6e-16 (alpha.0.bias)    9.6e-14 (decoder 0.weight)      8.8e-13   9.5e-14 (autoencoder_loss)
original_dirichlet_s0   2.3e-15    3.2e-15 (alpha.0.weight)  2.2e-13 (decoder 0.weight)      2.1e-13   3.4e-14 (autoencoder_loss)
two_layers-dirichlet    1.8e-15    3.5e-15 (phi_from b1)     9.4e-16 (decoder 2.bias)        2.6e-16   6.0e-16 (jacobian_loss)
two_layers-mixed        6.4e-16    3.2e-16 (update b1)       5.2e-16 (decoder 0.weight)      1.8e-16   1.1e-15 (jacobian_loss)
======================  =========  ========================  ==============================  ========  ===========================

* residual and A^T r (test 1): 250 x 1.3e-16 = 3.3e-14 off the structure limits and 250 x 5.1e-16 = 1.3e-13 on them are covered by
  ``GATE`` (1e-13, 1e-12) and ``GATE_LIMITS`` (2.7e-13, 1.4e-12) of tests/test_gpu_f64_deriv.py, reused; the duality defect
  |<w, A u> - <A^T w, u>| / (|w| |A u|) is held to the same relative figure (250 x 2.1e-16 = 5.3e-14 is inside it).
* mse (test 2): the loss 250 x 1.3e-14 = 3.3e-12 (``GATE_MSE``); the gradient is row-local and held to the 1e-13 of
  tests/test_gpu_f64.py.
* the step at a given state (test 3): matrices 250 x 2.3e-15 = 5.8e-13 and vectors 250 x 6.1e-15 = 1.5e-12 are covered by
  ``GATE_MATRIX`` (1.9e-12) and ``GATE_VECTOR`` (3.3e-11) of tests/test_gpu_f64_pgrad.py, reused.  The autoencoder's tensors are not
  covered by its ``GATE_MLP`` (1.1e-12): on a trained fixture the residual r = A u - y is what is left of a cancellation, its
  summation order moves it by 1e-12 relative, and the decoder's gradient and ``grad_h`` are linear in r.  Their gates are their own:
  ``GATE_AE`` = 250 x 3.2e-13 = 8.0e-11, ``GATE_GRAD_H`` = 250 x 1.0e-12 = 2.5e-10, and the loss scalars ``GATE_LOSS`` =
  250 x 9.5e-14 = 2.4e-11.
* the step with its own solves (test 4): the oracle step at tolerances 1e-10 against 1e-11 (fixtures; h* moves by <= 1.2e-9, y by
  <= 5.1e-7): matrices 5.0e-7 (update W1, hex13_dirichlet_s0), vectors 5.3e-7 (phi_to b2), autoencoder tensors 2.3e-6 (encoder
  0.weight), loss scalars 1.1e-7 (residual_loss).  That is the solver's own share; a device solve stopping at 1e-11 may sit anywhere
  within the tolerance ball, so the gates are 10 x those: 5.0e-6, 5.3e-6, 2.3e-5, 1.1e-6.  h* is held to the 5e-9 of
  ``test_converged_against_stored_truth``.
* the fp32 step against the new truth (test 5): the rule tests/test_gpu_gradients_at_scale.py uses for parameter gradients,
  ``limit_graphs.check_params`` with ``TAU_PGRAD`` = 2e-5 and the float32 oracle's own error as e32.
* d psi / dH_init of the backward of the VJP (test 7): Dirichlet rows of the arrays that ``GATE_DH`` of
  tests/test_gpu_f64_vjp_backward.py (250 x 2.8e-15) holds, reused.
No gate is taken from the device's output.  Measured on an MI355X with these gates (worst case over the file): residual / A^T w
1.4e-16 off the limits, 5.0e-16 on them (slots256 dirichlet), duality defect 2.1e-16 (line1); mse 2.2e-16; the step at a given state:
matrices 1.2e-14 (hex13_dirichlet_s0, phi_to W2), vectors 2.7e-14 (original_dirichlet_s0, alpha.0.weight), autoencoder tensors
4.1e-13 (hex13_dirichlet_s0, decoder 0.weight), grad_h 1.6e-12, loss scalars 4.2e-14 (residual_loss), the hook's residual within
0.5 % of the oracle's ``lowest``; with its own solves: 4.7e-8 / 4.7e-8 / 9.8e-8, loss scalars 1.8e-8, h* 3.6e-11 - 2.2e-10 from the
stored truth; d psi / dH_init 1.2e-15; the fp32 step: worst tensor e 1.9e-4 / 1.0e-4 / 3.7e-4 (decoder tensors; float32 oracle
7.2e-5 / 1.0e-4 / 1.3e-4) on hex13_dirichlet_s0 / hex13_mixed_s1 / original_dirichlet_s0, every tensor inside the rule.

What the step's composition had to gain.  A multi-layer dirichlet block copies the Dirichlet rows of ``H_init`` into every layer state
and evaluates its Jacobian there, so the regulariser reaches the encoder through ``H_init`` as well as f's parameters; without that
path the encoder tensors of two_layers-dirichlet sit 3.0e-4 - 3.9e-4 from the oracle.  ``psignn_f64_vjp_backward_init`` supplies it.
"""
import math

import pytest
import torch

import limit_graphs as lg
import train_step_ref as ts
import vjp_backward_cases as vb
from conftest import load_case, pkg, rel_l2
from test_gpu_f64_deriv import GATE, GATE_LIMITS
from test_gpu_f64_pgrad import GATE_MATRIX, GATE_VECTOR, TAU_PGRAD
from test_gpu_f64_vjp_backward import GATE_DH
from test_gpu_training import _model

pytestmark = pytest.mark.gpu

GATE_MSE = 250 * 1.3e-14
GATE_MSE_GRAD = 1e-13
GATE_AE = 250 * 3.2e-13
GATE_GRAD_H = 250 * 1.0e-12
GATE_LOSS = 250 * 9.5e-14
CLASS_GATE = {"matrix": GATE_MATRIX, "vector": GATE_VECTOR, "mlp": GATE_AE}
SOLVE_GATE = {"matrix": 10 * 5.0e-7, "vector": 10 * 5.3e-7, "mlp": 10 * 2.3e-6, "loss": 10 * 1.1e-7}
OUT_KEYS = {"loss", "loss_dic", "grads", "h_star", "new_h", "u", "grad_h", "y", "forward", "adjoint"}
# test 5: tensors left out of the fp32 rule.  Only the two cancelling tensors of the gate may ever stand here, and only with a figure
# in DESIGN section 7.
FP32_LEFT_OUT = ()


def _close(got, want, what, gate):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    rel, mx = rel_l2(got, want), float((got - want).abs().max())
    print(f"F64TS {what}: rel L2 {rel:.2e} max-abs {mx:.2e}")
    assert rel <= gate[0] and mx <= gate[1], (what, rel, mx)


def _check_grads(got, want, what, gates):
    """Every tensor of the state dict within the gate of its class; where autograd leaves nothing the device leaves exact zeros."""
    assert list(got) == list(want), (what, set(got) ^ set(want))
    bad, zeros = {}, 0
    for k, t in want.items():
        g = got[k]
        assert g.dtype == torch.float64 and g.shape == t.shape, (what, k, g.dtype, g.shape, t.shape)
        if not bool(t.any()):
            assert not bool(g.any()), (what, k, "the oracle leaves zeros, the device must leave exact zeros")
            zeros += 1
            continue
        c = ts.tensor_class(k, t)
        r = ts.rel(g, t)
        print(f"F64TS {what} {k}: rel L2 {r:.2e} ({c})")
        if not r <= gates[c]:
            bad[k] = (r, gates[c])
    assert not bad, (what, bad)
    return zeros


def _check_losses(out, o, what, gate):
    assert list(out["loss_dic"]) == ts.LOSS_KEYS and all(isinstance(v, float) for v in out["loss_dic"].values())
    for k in ts.LOSS_KEYS + ["loss"]:
        a, b = (out["loss"], float(o["loss"])) if k == "loss" else (out["loss_dic"][k], float(o["loss_dic"][k]))
        r = abs(a - b) / abs(b) if b != 0 else abs(a - b)
        print(f"F64TS {what} {k}: {a:.15e} (oracle {b:.15e}) rel {r:.2e}")
        assert r <= gate, (what, k, a, b, r)


def _same_step(a, b):
    return (a["loss"] == b["loss"] and a["loss_dic"] == b["loss_dic"] and all(torch.equal(a["grads"][k], b["grads"][k]) for k in a["grads"])
            and all(torch.equal(a[k], b[k]) for k in ("h_star", "new_h", "u", "grad_h", "y")))


# ----------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("name", ts.RESIDUAL_NAMES)
def test_residual_and_its_transpose(name, dev):
    eng = pkg("engine")
    mesh, tile_target, u, w = ts.residual_case(name)
    md = mesh.to(dev)
    plan = eng.MeshPlan(md, tile_target=tile_target)
    N = mesh.num_nodes
    if name == "hex60":
        assert -(-N // 256) > 40 and N % 256 != 0   # many blocks, a ragged tail
    a64, y64 = mesh.a_ij.double(), mesh.y.double()
    want_r, want_t = ts.residual_ref(mesh.edge_index, a64, u, y64), ts.residual_t_ref(mesh.edge_index, a64, w)
    ud, wd = u.to(dev), w.to(dev)
    r, t = eng.residual64(plan, md.a_ij, ud, md.y), eng.residual64_t(plan, md.a_ij, wd)
    assert r.dtype == t.dtype == torch.float64 and r.shape == t.shape == (N, 1)
    gate = GATE_LIMITS if name.split("-")[0] in ts.LIMITS else GATE
    _close(r, want_r, f"{name} A u - y", gate)
    _close(t, want_t, f"{name} A^T w", gate)
    Au = r.cpu() + y64
    dual = abs(float((w * Au).sum()) - float((t.cpu() * u).sum())) / (float(w.norm()) * float(Au.norm()))
    print(f"F64TS {name} duality defect {dual:.2e}")
    assert dual <= gate[0], (name, dual)
    # the same call gives the same bits; float32 inputs are widened exactly (the fixtures' a_ij and y are float32 already)
    assert torch.equal(r, eng.residual64(plan, md.a_ij, ud, md.y)) and torch.equal(t, eng.residual64_t(plan, md.a_ij, wd))
    assert torch.equal(r, eng.residual64(plan, md.a_ij.double(), ud, md.y.double()))
    assert torch.equal(t, eng.residual64_t(plan, md.a_ij.double().reshape(-1), wd.reshape(-1)))
    assert torch.equal(eng.residual64(plan, md.a_ij, ud.float(), md.y), eng.residual64(plan, md.a_ij, ud.float().double(), md.y))


# ----------------------------------------------------------------------------------------------------------------- 2
def _mse_lengths():
    chunk = 1024   # psignn_mse_f64_chunk(), asserted in the test
    return [1, chunk - 1, chunk, chunk + 1, 256 * chunk + 1, 109810]


@pytest.mark.parametrize("n", _mse_lengths())
def test_mse64(n, dev):
    eng = pkg("engine")
    assert pkg("_native").lib().psignn_mse_f64_chunk() == 1024
    gen = torch.Generator().manual_seed(70 + n % 97)
    shape = (10981, 10) if n == 109810 else (n,)
    a, b = (torch.randn(shape, generator=gen, dtype=torch.float64) for _ in range(2))
    ad, bd = a.to(dev), b.to(dev)
    for with_b in (True, False):
        diff = a - b if with_b else a
        want, want_g = float(torch.mean(diff ** 2)), 2 * diff / n
        for need_grad in (True, False):
            loss, grad = eng.mse64(ad, bd if with_b else None, need_grad=need_grad)
            assert loss.dtype == torch.float64 and loss.dim() == 0 and loss.is_cuda
            r = abs(float(loss) - want) / want
            print(f"F64TS mse n {n} b {with_b} grad {need_grad}: {float(loss):.15e} rel {r:.2e}")
            assert r <= GATE_MSE, (n, with_b, need_grad, r)
            again = eng.mse64(ad, bd if with_b else None, need_grad=need_grad)
            assert torch.equal(loss, again[0])
            if need_grad:
                rg = ts.rel(grad, want_g)
                assert grad.shape == a.shape and grad.dtype == torch.float64 and rg <= GATE_MSE_GRAD, (n, with_b, rg)
                assert torch.equal(grad, again[1])
            else:
                assert grad is None and again[1] is None
    # float32 inputs are widened exactly
    assert torch.equal(eng.mse64(ad.float(), bd.float())[0], eng.mse64(ad.float().double(), bd.float().double())[0])


# ----------------------------------------------------------------------------------------------------------------- 3
_given = {}


def _step_at_the_oracles_state(name, dev):
    if name not in _given:
        o = ts.oracle_at(name)
        md = o["mesh"].to(dev)
        hs, y = o["fw"]["result"].detach(), o["bw"]["result"].detach()
        out = pkg("engine").train_step64(md, o["sd"], h_star=hs.to(dev), y=y.to(dev), probe=o["probe"].to(dev), jac_weight=1.0)
        _given[name] = (o, md, hs, y, out)
    return _given[name]


@pytest.mark.parametrize("name", ts.STEP_NAMES)
def test_step_at_a_given_state(name, dev):
    eng = pkg("engine")
    o, md, hs, y, out = _step_at_the_oracles_state(name, dev)
    print(f"F64TS {name}: oracle fw nstep {o['fw']['nstep']} lowest {o['fw']['lowest']:.2e}, bw nstep {o['bw']['nstep']} "
          f"lowest {o['bw']['lowest']:.2e}")
    assert set(out) == OUT_KEYS and out["forward"] is None and out["adjoint"] is None
    assert list(out["grads"]) == list(o["sd"])   # exactly the state dict's keys
    zeros = _check_grads(out["grads"], o["grads"], name, CLASS_GATE)
    if name == "two_layers-mixed":
        assert zeros == 12   # only the last iteration of a mixed block reaches the output
    _check_losses(out, o, name, GATE_LOSS)
    assert isinstance(out["loss"], float) and math.isfinite(out["loss"])
    assert torch.equal(out["y"], y.to(dev)) and torch.equal(out["h_star"], hs.to(dev))
    # the cotangent the hook receives, against the restated step's
    _, _, _, want_gh = ts.train_step_ref(o["sd"], o["mesh"], hs, y, o["probe"], 1.0)
    r = ts.rel(out["grad_h"], want_gh)
    print(f"F64TS {name} grad_h: rel L2 {r:.2e}")
    assert out["grad_h"].dtype == torch.float64 and r <= GATE_GRAD_H, (name, r)
    # y solves y = J^T y + grad_h as well as the oracle's solve left it: its `lowest`, plus what the product's and grad_h's gates allow
    plan = eng.plan_for(md)
    fmap = eng.FixedPointMap64(plan, eng.PackedWeights64(o["sd"]), eng.mlp2_64(md.x, *[o["sd"][f"autoencoder.encoder.mlp.mlp.{i}.{p}"]
                               for i, p in ((0, "weight"), (0, "bias"), (2, "weight"), (2, "bias"))]), md.prb_data, md.edge_attr,
                               getattr(md, "unit_normal_vector", None))
    try:
        yd = y.to(dev)
        jt, fy = fmap.vjp(hs.to(dev), yd), fmap.vjp(hs.to(dev), yd, out["grad_h"])
    finally:
        fmap.close()
    den = float(fy.norm()) + 1e-9
    rel = float((fy - yd).norm()) / den
    allow = o["bw"]["lowest"] * (1 + 1e-6) + (GATE[0] * float(jt.norm()) + GATE_GRAD_H * float(out["grad_h"].norm())) / den
    print(f"F64TS {name} hook residual {rel:.3e} (oracle lowest {o['bw']['lowest']:.3e}, allowed {allow:.3e})")
    assert rel <= allow, (name, rel, allow)
    # the same call gives the same bits
    again = eng.train_step64(md, o["sd"], h_star=hs.to(dev), y=y.to(dev), probe=o["probe"].to(dev), jac_weight=1.0)
    assert _same_step(out, again), name
    if name == "hex13_mixed_s1":   # a probe without a weight still reports the regulariser; no probe reports 0
        off = eng.train_step64(md, o["sd"], h_star=hs.to(dev), y=y.to(dev), probe=o["probe"].to(dev))
        assert off["loss_dic"]["jacobian_loss"] == out["loss_dic"]["jacobian_loss"]
        none = eng.train_step64(md, o["sd"], h_star=hs.to(dev), y=y.to(dev))
        assert none["loss_dic"]["jacobian_loss"] == 0.0 and none["loss"] == off["loss"]
        assert all(torch.equal(none["grads"][k], off["grads"][k]) for k in off["grads"])
        bare = md.clone()
        del bare.sol
        assert math.isnan(eng.train_step64(bare, o["sd"], h_star=hs.to(dev), y=y.to(dev))["loss_dic"]["mse_loss"])


# ----------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("name", ts.FIXTURES)
def test_step_with_its_own_solves(name, dev):
    eng = pkg("engine")
    o = ts.oracle_at(name)
    md = o["mesh"].to(dev)
    out = eng.train_step64(md, o["sd"], probe=o["probe"].to(dev), jac_weight=1.0)
    assert set(out) == OUT_KEYS
    fw, bw = out["forward"], out["adjoint"]
    assert fw is not None and bw is not None and torch.equal(fw["result"], out["h_star"]) and torch.equal(bw["result"], out["y"])
    print(f"F64TS {name}: forward n_iter {fw['n_iter']} lowest {fw['lowest']:.2e}; adjoint products {bw['nstep']} lowest "
          f"{bw['lowest']:.2e} stop {bw['stop']}")
    assert fw["lowest"] < 1e-11 and bw["lowest"] < 1e-11
    dist = rel_l2(out["h_star"], load_case(name)[0]["fp64_result"])
    print(f"F64TS {name}: distance of h* to the stored fp64_result {dist:.2e}")
    assert dist <= 5e-9
    _check_grads(out["grads"], o["grads"], f"{name} own solves", SOLVE_GATE)
    _check_losses(out, o, f"{name} own solves", SOLVE_GATE["loss"])


# ----------------------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("name", ts.FIXTURES)
def test_fp32_training_step_against_the_float64_step(name, dev):
    """``ModelDEQDSS`` in train mode (the set-up of tests/test_gpu_training.py, ``jac_weight`` 1): its gradients against
    ``train_step64`` at its own ``last_forward`` / ``last_backward`` / ``last_probe``, by the rule of
    tests/test_gpu_gradients_at_scale.py; the float32 oracle at the same state is e32."""
    eng = pkg("engine")
    sd, mesh, _, _ = ts.step_case(name)
    md = mesh.to(dev)
    net = _model(sd, dev, fw_tol=1e-7, fw_thres=600).train()
    u, ld = net(md)
    (ld["residual_loss"] + 1.0 * ld["jacobian_loss"] + ld["encoder_loss"] + ld["autoencoder_loss"]).backward()
    got = {k: p.grad for k, p in net.named_parameters()}
    hs, y, probe = net.deqdss.last_forward["result"], net.deqdss.last_backward["result"], net.deqdss.last_probe
    truth = eng.train_step64(md, sd, h_star=hs, y=y, probe=probe, jac_weight=1.0)
    want64 = {k: t.cpu() for k, t in truth["grads"].items()}
    assert set(got) == set(want64)
    l32, d32, want32, _ = ts.train_step_ref(sd, mesh, hs.cpu(), y.cpu(), probe.cpu(), 1.0, dtype=torch.float32)
    for k in ("residual_loss", "encoder_loss", "autoencoder_loss", "jacobian_loss"):
        print(f"F64TS {name} fp32 {k}: {float(ld[k].detach()):.8e} float64 {truth['loss_dic'][k]:.8e} float32 oracle {float(d32[k]):.8e}")
    scale = max(float(t.norm()) for t in want64.values())
    for k, t in want64.items():
        den = max(float(t.norm()), 1e-4 * scale)
        print(f"F64TS {name} fp32 {k}: e {float((got[k].cpu().double() - t).norm()) / den:.2e} "
              f"e32 {float((want32[k].double() - t).norm()) / den:.2e}")
    keep = [k for k in want64 if not any(k.endswith(x) for x in FP32_LEFT_OUT)]
    assert len(keep) >= len(want64) - 2 and all(x in ("alpha.0.weight", "alpha.0.bias") for x in FP32_LEFT_OUT)
    e, e32 = lg.check_params(got, {k: want64[k] for k in keep}, want32, TAU_PGRAD, f"{name} fp32 training step vs train_step64")
    print(f"F64TS {name} fp32 training step vs train_step64: worst e {e:.2e} (float32 oracle {e32:.2e})")


# ----------------------------------------------------------------------------------------------------------------- 6
def test_refusals_on_the_device(dev):
    """Aliasing, NULL, an empty length and a workspace one double short are error codes, and the message names the bytes; the Python
    side refuses a wrong ``a_ij``, a weight without a probe and another latent width before any native call."""
    nat, eng = pkg("_native"), pkg("engine")
    lib, ptr = nat.lib(), nat.ptr
    err = lambda: lib.psignn_last_error().decode()
    _, mesh = load_case("hex13_dirichlet_s0")
    md = mesh.to(dev)
    plan = eng.plan_for(md)
    N = plan.N
    a = md.a_ij.double().reshape(-1).contiguous()
    u, y, r, t = (torch.zeros(N, dtype=torch.float64, device=dev) for _ in range(4))
    assert lib.psignn_residual_f64(plan.handle, ptr(a), ptr(u), ptr(y), ptr(u), None) < 0 and "alias" in err()
    assert lib.psignn_residual_f64(plan.handle, ptr(a), ptr(u), ptr(y), ptr(y), None) < 0 and "alias" in err()
    assert lib.psignn_residual_f64(plan.handle, None, ptr(u), ptr(y), ptr(r), None) < 0 and "NULL" in err()
    assert lib.psignn_residual_f64(None, ptr(a), ptr(u), ptr(y), ptr(r), None) < 0 and "NULL" in err()
    assert lib.psignn_residual_f64(plan.handle, ptr(a), ptr(u), ptr(y), ptr(r), None) == 0
    assert lib.psignn_residual_t_f64(plan.handle, ptr(a), ptr(r), ptr(r), None) < 0 and "alias" in err()
    assert lib.psignn_residual_t_f64(plan.handle, ptr(a), ptr(r), None, None) < 0 and "NULL" in err()
    assert lib.psignn_residual_t_f64(plan.handle, ptr(a), ptr(r), ptr(t), None) == 0
    chunk = lib.psignn_mse_f64_chunk()
    n = 2 * chunk + 1
    need = lib.psignn_mse_f64_workspace_doubles(n)
    assert need == 3
    x, z, g = (torch.zeros(n, dtype=torch.float64, device=dev) for _ in range(3))
    loss, work = torch.zeros((), dtype=torch.float64, device=dev), torch.zeros(need, dtype=torch.float64, device=dev)
    mse = lambda a_, b_, n_, l_, g_, w_, nw: lib.psignn_mse_f64(a_, b_, n_, float(max(n_, 1)), l_, g_, w_, nw, None)
    assert mse(ptr(x), ptr(z), n, ptr(loss), ptr(x), ptr(work), need) < 0 and "alias" in err()
    assert mse(ptr(x), ptr(z), n, ptr(loss), ptr(z), ptr(work), need) < 0 and "alias" in err()
    assert mse(None, ptr(z), n, ptr(loss), ptr(g), ptr(work), need) < 0 and "NULL" in err()
    assert mse(ptr(x), ptr(z), n, None, ptr(g), ptr(work), need) < 0 and "NULL" in err()
    assert mse(ptr(x), ptr(z), 0, ptr(loss), ptr(g), ptr(work), need) < 0 and "n_elems" in err()
    assert mse(ptr(x), ptr(z), n, ptr(loss), ptr(g), ptr(work), need - 1) < 0 and f"{need * 8} bytes" in err()
    assert mse(ptr(x), ptr(z), n, ptr(loss), ptr(g), None, need) < 0 and f"{need * 8} bytes" in err()
    assert mse(ptr(x), ptr(z), n, ptr(loss), ptr(g), ptr(work), need) == 0 and mse(ptr(x), None, n, ptr(loss), None, ptr(work), need) == 0
    torch.cuda.synchronize(dev)
    with pytest.raises(nat.NativeError, match="a_ij has"):
        eng.residual64(plan, md.a_ij[:-1], u, y)
    with pytest.raises(nat.NativeError, match="a_ij has"):
        eng.residual64_t(plan, torch.cat([md.a_ij, md.a_ij]), r)
    sd = ts.step_case("hex13_dirichlet_s0")[0]
    hs = torch.zeros(N, 10, dtype=torch.float64, device=dev)
    with pytest.raises(nat.NativeError, match="needs a probe"):
        eng.train_step64(md, sd, h_star=hs, y=hs, jac_weight=1.0)
    wide = pkg("model_psignn").ModelPSIGNN(dict(latent_dim=8, n_layers=1)).state_dict()
    with pytest.raises(nat.NativeError, match="forward inference only"):
        eng.train_step64(md, wide, h_star=hs, y=hs)


# ----------------------------------------------------------------------------------------------------------------- 7
@pytest.mark.parametrize("name", ["two_layers-dirichlet", "two_layers-mixed", "hex13_dirichlet_s0@h0"])
def test_vjp_backward_init(name, dev):
    """``d psi / dH_init`` of ``psi = <Gbar, J_f(H)^T V>`` against autograd on the oracle; the first three outputs have the bits of
    ``vjp_backward``.  Only a multi-layer dirichlet block has a Jacobian that depends on ``H_init``."""
    from oracle import psignn_oracle as orc
    from test_gpu_f64 import Problem
    c = vb.make(name)
    p = Problem(c.mesh, c.sd, dev, tile_target=c.tile_target, h0=c.h0)
    Hd, Vd, Gd = c.H.to(dev), c.V.to(dev), c.Gbar.to(dev)
    named, dh, jtv, dinit = p.fmap.vjp_backward_init(Hd, Vd, Gd)
    base = p.fmap.vjp_backward(Hd, Vd, Gd)
    assert all(torch.equal(named[k], base[0][k]) for k in named) and torch.equal(dh, base[1]) and torch.equal(jtv, base[2])
    with ts.default_dtype(torch.float64):
        hh = c.H.clone().requires_grad_(True)
        h0 = p.h0.clone().requires_grad_(True)
        out = orc.function_forward(p.s64, hh, h0, p.m64)
        g = torch.autograd.grad(out, hh, c.V, create_graph=True)[0]
        want = torch.autograd.grad((g * c.Gbar).sum(), h0, allow_unused=True)[0]
    assert dinit.dtype == torch.float64 and dinit.shape == c.H.shape
    if name == "two_layers-dirichlet":
        r = ts.rel(dinit, want)
        print(f"F64TS {name} d psi / dH_init: rel L2 {r:.2e}")
        assert bool(want.any()) and r <= GATE_DH, (name, r)
        assert not bool(dinit.cpu()[want == 0].any())   # rows that are not Dirichlet rows: exact zeros
        assert torch.equal(dinit, p.fmap.vjp_backward_init(Hd, Vd, Gd)[3])
    else:
        assert (want is None or not bool(want.any())) and not bool(dinit.any()), name
