"""bf16 storage of the Broyden solver's rank-one pairs (``DeviceBroyden(..., history_dtype=torch.bfloat16)``,
``psignn_broyden_create_opts(history = 1)``).

Semantics under test: each stored pair is rounded to bf16 (nearest even) when it is written, and every quantity derived from a
new pair takes the rounded value -- vT_b = bf16(vT) gives s = vT_b . dg, beta = vT_b . g and V_k; u_b = bf16(D1 / s) gives U_k and
the update D2 - u_b beta -- so that B = -I + sum U_j V_j^T holds exactly over the stored bf16 values.  Arithmetic, iterate and
update stay fp32.  The per-iteration checks therefore recompute each step in float64 from the device's own (bf16) stored pairs,
as ``recurrences._check_iteration`` does for fp32 pairs: V_k and U_k may differ from the float64 values by the bf16 rounding
(2^-8 relative) on top of the fp32 tolerance, the update keeps the fp32 tolerance (it would miss it by ~2^-9 |u beta| had the
kernel used the unrounded u or vT)."""
import ctypes as C
import os
import weakref

import numpy as np
import pytest
import torch

from conftest import CASES, load_case, load_weights, pkg, rel_l2
from oracle import psignn_oracle as orc
from recurrences import EPS32, _scale, tail
from test_gpu_solver_forms import K, _linear, _Recorder, _setenv

pytestmark = pytest.mark.gpu

BF = 2.0 ** -8      # bf16 unit roundoff: 8 significant bits, round to nearest
BF16 = torch.bfloat16


# ---------------------------------------------------------------------------------------------------------- bf16 recurrences
def _check_on(U32m, V32m, U, V, dx, dg, g, Vk, Uk, upd_next, where, c_vT, c_D1, c_D2, glob=None):
    """recurrences._check_iteration_on with the stored V_k, U_k allowed their bf16 rounding; the update check unchanged."""
    dxd, dgd, gd = dx.double(), dg.double(), g.double()
    vT = -dxd + c_vT[0] @ V
    vT32 = -dx + c_vT[1] @ V32m
    e = float((Vk.double() - vT).norm())
    tv = BF * float(vT.norm()) + 16 * _scale(vT, vT32)
    assert e <= tv, (where, "vT", e, tv)
    D1 = dxd + dgd - c_D1[0] @ U
    D1_32 = dx + dg - c_D1[1] @ U32m
    Ukd = Uk.double()
    tol_dir = 16 * _scale(D1, D1_32) / float(D1.norm())
    if glob is None:
        proj = float(D1 @ Ukd) / float(D1 @ D1)
        rem = float((Ukd - proj * D1).norm())
        assert rem <= (BF + tol_dir) * float(Ukd.norm()), (where, "U_k direction", rem / float(Ukd.norm()), tol_dir)
        s64 = float(Vk.double() @ dgd)
        s_abs = float((Vk.double() * dgd).abs().sum())
        assert abs(1.0 / proj - s64) <= 16 * EPS32 * s_abs + (2 * BF + 4 * tol_dir) * abs(s64), (where, "s", 1.0 / proj, s64)
    else:
        proj, _, tol_dir_all, _ = glob
        rem = float((Ukd - proj * D1).norm())
        assert rem <= (BF + tol_dir + tol_dir_all) * float(Ukd.norm()), (where, "U_k direction", rem / float(Ukd.norm()))
    # update = D2 - u_b beta with the STORED u_b: fp32 tolerance
    D2 = gd - c_D2[0] @ U
    D2_32 = g - c_D2[1] @ U32m
    r = D2 - upd_next.double()
    tol2 = 16 * _scale(D2, D2_32)
    if glob is None:
        beta = float(r @ Ukd) / float(Ukd @ Ukd)
        rem2 = float((r - beta * Ukd).norm())
        tol2 += 8 * EPS32 * (float(D2.norm()) + abs(beta) * float(Ukd.norm()))
        assert rem2 <= tol2, (where, "update", rem2, tol2)
        b64 = float(Vk.double() @ gd)          # beta = vT_b . g with the STORED vT_b: fp32 tolerance
        b_abs = float((Vk.double() * gd).abs().sum())
        assert abs(beta - b64) <= 16 * EPS32 * b_abs + 4 * (tol2 / float(Ukd.norm())), (where, "beta", beta, b64, b_abs)
        return proj, beta, tol_dir, tol2 / float(Ukd.norm())
    _, beta, _, dbeta = glob
    rem2 = float((r - beta * Ukd).norm())
    tol2 += 8 * EPS32 * (float(D2.norm()) + abs(beta) * float(Ukd.norm())) + dbeta * float(Ukd.norm())
    assert rem2 <= tol2, (where, "update", rem2, tol2)


def _check_iteration_bf16(U32, V32, U, V, dx, dg, g, Vk, Uk, upd_next, where):
    dxd, dgd, gd = dx.double(), dg.double(), g.double()
    c_vT, c_D1, c_D2 = (U @ dxd, U32 @ dx), (V @ dgd, V32 @ dg), (V @ gd, V32 @ g)
    glob = _check_on(U32, V32, U, V, dx, dg, g, Vk, Uk, upd_next, where, c_vT, c_D1, c_D2)
    sl = tail(dx.numel())
    _check_on(U32[:, sl], V32[:, sl], U[:, sl], V[:, sl], dx[sl], dg[sl], g[sl], Vk[sl], Uk[sl], upd_next[sl],
              f"{where} tail", c_vT, c_D1, c_D2, glob)


def _run_recorded(eng, f, x0, history_dtype=BF16):
    rec = _Recorder(f)
    sv = eng.DeviceBroyden(threshold=K, keep_trace=True, n_elems=x0.numel(), seq_len=x0.shape[1], device=x0.device,
                           history_dtype=history_dtype)
    rec.solver = sv
    out = sv.solve_callable(rec, x0, 0.0)
    assert out["n_iter"] == K and out["stop_reason"] == 0, (out["n_iter"], out["stop_reason"])
    rec.DX.append(sv.pair(0, x0, "update"))
    return rec, sv, out


def _pairs(sv, like, n):
    U = torch.stack([sv.pair(j, like, "U").reshape(-1).cpu() for j in range(n)])
    V = torch.stack([sv.pair(j, like, "V").reshape(-1).cpu() for j in range(n)])
    return U, V


def _check_run(rec, sv, its, label):
    X, DX = rec.X, rec.DX
    assert len(X) == K + 1 and len(DX) == K + 1
    for i in (1, K // 2, K):
        assert torch.equal(sv.iterate(i, X[0]), X[i])
    Ucpu, Vcpu = _pairs(sv, X[0], max(its) + 1)
    # every stored value IS a bf16 value, widened exactly
    assert torch.equal(Ucpu, Ucpu.to(BF16).float()) and torch.equal(Vcpu, Vcpu.to(BF16).float()), label
    U64, V64 = Ucpu.double(), Vcpu.double()
    G = {}

    def gof(i):
        if i not in G:
            G[i] = (rec.f(X[i]) - X[i]).reshape(-1).cpu()
        return G[i]

    for it in its:
        g_new, g_old = gof(it + 1), gof(it)
        _check_iteration_bf16(Ucpu[:it], Vcpu[:it], U64[:it], V64[:it], DX[it].reshape(-1).cpu(), g_new - g_old, g_new,
                              Vcpu[it], Ucpu[it], DX[it + 1].reshape(-1).cpu(), f"{label} it={it}")


def _ld(M, q):
    return (M + q - 1) // q * q


SHAPES = {"4wide": (100000, (0, 1, 5, 9, 17, 25, 33, 46)), "16wide": (320000, (0, 1, 9, 24, 25, 46)),
          "ragged": (100001, (0, 1, 9, 25, 46))}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_bf16_pairs_storage_and_recurrences(shape, dev, monkeypatch):
    """f(x) = c x + b through the generic-callable path, natural shapes: (100 000, 10) runs the 4-float three-sweep form,
    (320 000, 10) the 16-float one, (100 001, 10) a ragged last lane.  The bf16 solver holds half the pair bytes of the fp32
    one (rows padded to 128 elements instead of 64), every pair it hands out is a bf16 value, and every checked iteration
    satisfies the bf16-history recurrences (whole vector and tail)."""
    eng = pkg("engine")
    _setenv(monkeypatch, {})
    N, its = SHAPES[shape]
    c, b, x0 = _linear(N, 0.995, dev)
    cd, bd, x0d = c.to(dev), b.to(dev), x0.to(dev)
    f = lambda x: cd * x + bd
    M = x0d.numel()
    # storage
    s32 = eng.DeviceBroyden(threshold=K, keep_trace=False, n_elems=M, seq_len=10, device=dev)
    s16 = eng.DeviceBroyden(threshold=K, keep_trace=False, n_elems=M, seq_len=10, device=dev, history_dtype=BF16)
    assert s16.nbytes == s32.nbytes - 2 * K * (4 * _ld(M, 64) - 2 * _ld(M, 128)), (s16.nbytes, s32.nbytes)
    o32 = s32.solve_callable(f, x0d, 0.0)
    U32, V32 = _pairs(s32, x0d, 8)
    assert not (torch.equal(U32, U32.to(BF16).float()) and torch.equal(V32, V32.to(BF16).float()))   # fp32 pairs are not bf16
    s32.close()
    s16.close()
    rec, sv, out = _run_recorded(eng, f, x0d)
    with torch.no_grad():
        ref = orc.broyden(lambda x: c * x + b, x0, threshold=6, eps=0.0)
    # the first iterations follow the fp32 reference to within the pairs' rounding
    np.testing.assert_allclose(out["rel_trace"][:3], ref["rel_trace"][:3], rtol=2e-2)
    _check_run(rec, sv, its, f"{shape}/bf16")
    print(f"{shape}: lowest after {K} iterations fp32 {o32['lowest']:.3e} bf16 {out['lowest']:.3e}")
    sv.close()


@pytest.mark.parametrize("N", [1, 25, 409])
def test_bf16_pairs_on_vectors_shorter_than_a_block(N, dev, monkeypatch):
    """M = 10, 250, 4 090: recurrences while k is well below M; a well-conditioned problem converges to b / (1 - c)."""
    eng, solver = pkg("engine"), pkg("utilities.solver")
    _setenv(monkeypatch, {})
    M = N * 10
    c, b, x0 = _linear(N, 0.995, dev, seed=3)
    cd, bd, x0d = c.to(dev), b.to(dev), x0.to(dev)
    rec, sv, out = _run_recorded(eng, lambda x: cd * x + bd, x0d)
    _check_run(rec, sv, [i for i in (0, 1, 2, 3, 5, 9, 16, 24, 25, 26) if i <= M // 3], f"M={M}")
    sv.close()
    c, b, x0 = _linear(N, 0.5, dev, seed=4)
    cd, bd, x0d = c.to(dev), b.to(dev), x0.to(dev)
    o = solver.broyden(lambda x: cd * x + bd, x0d, threshold=K, eps=0.0, keep_trace=False, history_dtype=BF16)
    assert bool(torch.isfinite(o["result"]).all())
    assert rel_l2(o["result"], b / (1 - c)) < 1e-6 and o["lowest"] < 2e-7, (M, rel_l2(o["result"], b / (1 - c)), o["lowest"])


# ---------------------------------------------------------------------------------------------------------- convergence
def _bind(name, dev):
    g, mesh = load_case(name)
    sd = load_weights(CASES[name])
    eng = pkg("engine")
    md = mesh.to(dev)
    fmap = eng.FixedPointMap(eng.plan_for(md), eng.PackedWeights(sd, dev), torch.from_numpy(g["h0"]).to(dev), md.prb_data,
                             getattr(md, "unit_normal_vector", None))
    return g, mesh, md, sd, fmap


# bf16-history solves of two fixtures that miss eps = 1e-7: hex13_mixed_s1 ends on the protective break (stop reason 3),
# hex26_dirichlet_s0 on the threshold (0); (stop_reason, n_iter, nstep of the lowest iterate, bound on its residual)
MEASURED_MISSES = {"hex13_mixed_s1": (3, 250, 123, 1.6e-6), "hex26_dirichlet_s0": (0, 1000, 247, 2.6e-5)}


def test_bf16_history_converges_to_the_fp64_fixed_point(dev, monkeypatch):
    """The four fixtures of the north-star test, on-device solve from the encoder state, threshold 1 000, eps 1e-7, bf16 pairs.
    original_dirichlet_s0 and hex13_dirichlet_s0: the stop test is met and h* lies within 1e-5 of the fp64 fixed point (measured
    on MI355X: 396 / 169 iterations against 149 / 157 with fp32 pairs).  The two others do NOT get there with bf16 pairs, and
    this test records it: hex13_mixed_s1 reaches 1.5e-6 at iteration 123, then the protective break at
    250; hex26_dirichlet_s0 stalls near 2.5e-5 and runs to the threshold (fp32 pairs: 1e-7 after 210 / 532).  The solves are
    bitwise reproducible, so these outcomes are asserted as measured -- stop reason, iterations, lowest step and a bound on the
    lowest residual -- and a change of behaviour either way fails the test.  And the
    closed-form problem (c <= 0.5) on (320 000, 10): b / (1 - c) within 1e-6 in 48 iterations.  Iteration counts of both
    histories are printed side by side."""
    solver = pkg("utilities.solver")
    _setenv(monkeypatch, {})
    for name in ("original_dirichlet_s0", "hex13_dirichlet_s0", "hex13_mixed_s1", "hex26_dirichlet_s0"):
        g, mesh, md, sd, fmap = _bind(name, dev)
        o32 = solver.broyden(fmap, fmap.h0, threshold=1000, eps=1e-7)
        o16 = solver.broyden(fmap, fmap.h0, threshold=1000, eps=1e-7, history_dtype=BF16)
        e32, e16 = rel_l2(o32["result"], g["fp64_result"]), rel_l2(o16["result"], g["fp64_result"])
        print(f"{name}: iterations fp32 {o32['n_iter']} bf16 {o16['n_iter']} (stop reasons {o32['stop_reason']} / "
              f"{o16['stop_reason']}, lowest {o32['lowest']:.2e} / {o16['lowest']:.2e} at {o32['nstep']} / {o16['nstep']}); "
              f"h* vs fp64 fp32 {e32:.2e} bf16 {e16:.2e}")
        if name in MEASURED_MISSES:   # (stop_reason, n_iter, nstep, bound on lowest) as measured
            reason, n_iter, nstep, low = MEASURED_MISSES[name]
            got = (o16["stop_reason"], o16["n_iter"], o16["nstep"])
            assert got == (reason, n_iter, nstep) and o16["lowest"] < low, (name, got, o16["lowest"])
            assert bool(torch.isfinite(o16["result"]).all()), name
            continue
        assert o16["lowest"] < 1e-7, (name, o16["lowest"], o16["n_iter"])
        assert e16 < 1e-5, (name, e16)
    c, b, x0 = _linear(320000, 0.5, dev, seed=2)
    cd, bd, x0d = c.to(dev), b.to(dev), x0.to(dev)
    for hd in (torch.float32, BF16):
        o = solver.broyden(lambda x: cd * x + bd, x0d, threshold=K, eps=0.0, keep_trace=False, history_dtype=hd)
        print(f"closed form (320000, 10), {hd}: lowest {o['lowest']:.2e} at iteration {o['nstep']}")
        assert rel_l2(o["result"], b / (1 - c)) < 1e-6, (hd, rel_l2(o["result"], b / (1 - c)))
        assert o["lowest"] < 2e-7 and bool(torch.isfinite(o["result"]).all()), (hd, o["lowest"])


# ---------------------------------------------------------------------------------------------------------- adjoint, training
def _deq_model(sd, dev, **kw):
    solver = pkg("utilities.solver")
    cfg = dict(latent_dim=10, n_layers=1, solver=solver.broyden, fw_tol=1e-7, fw_thres=600, bw_tol=1e-6, bw_thres=600)
    cfg.update(kw)
    net = pkg("model_psignn").ModelDEQDSS(cfg)
    net.load_state_dict(sd)
    return net.to(dev)


@pytest.mark.parametrize("linearize", [False, True])
def test_bf16_history_adjoint_solve(linearize, dev):
    """The implicit backward's on-device adjoint solve (test_gpu_parity.py::test_implicit_backward_solve's setup) with
    ``broyden_history_dtype = torch.bfloat16``, with and without ``bw_linearize``: converged, the adjoint equation holds with
    the ORACLE's VJP, and the solution agrees with the fp32-history one."""
    g, mesh, md, sd, fmap = _bind("hex13_dirichlet_s0", dev)
    h_star = torch.from_numpy(g["broyden_e7_result"])
    h0 = torch.from_numpy(g["h0"])
    grad = torch.randn(h_star.shape, generator=torch.Generator().manual_seed(9))
    net32 = _deq_model(sd, dev, bw_linearize=linearize)
    net16 = _deq_model(sd, dev, bw_linearize=linearize, broyden_history_dtype=BF16)
    o32 = net32.deqdss.implicit_backward(h_star.to(dev), h0.to(dev), md, grad.to(dev))
    o16 = net16.deqdss.implicit_backward(h_star.to(dev), h0.to(dev), md, grad.to(dev))
    assert net16.deqdss._bw_solver.history_dtype == BF16 and net32.deqdss._bw_solver.history_dtype == torch.float32
    print(f"adjoint (bw_linearize={linearize}): iterations fp32 {o32['n_iter']} bf16 {o16['n_iter']}")
    assert o16["lowest"] < 1e-6, o16["lowest"]
    y = o16["result"].cpu()
    r = orc.function_vjp(sd, h_star, h0, mesh, y) + grad - y
    assert float(r.norm() / y.norm()) < 1e-4
    assert rel_l2(o16["result"], o32["result"]) < 1e-3


def test_bf16_history_training_step_gradients(dev):
    """One training step (test_gpu_training.py::test_training_step_gradients, hex13_dirichlet_s0, draw 0) with bf16 pairs in
    the forward and the adjoint solve: every gradient tensor within the 1e-2 of the float64 truth that test allows any single
    fp32 run (a step's gradient is a chaotic sample; it is not compared with the fp32-history step)."""
    name = "hex13_dirichlet_s0"
    g, mesh = load_case(name)
    sd = load_weights(CASES[name])
    T = np.load(os.path.join(os.path.dirname(__file__), "golden", "grad_truth_fp64.npz"))
    net = _deq_model(sd, dev, fw_thres=600, bw_tol=1e-7, bw_thres=400, broyden_history_dtype=BF16).train()
    u, ld = net(mesh.to(dev))
    loss = ld["residual_loss"] + ld["encoder_loss"] + ld["autoencoder_loss"]
    loss.backward()
    assert net.deqdss._fw_solver.history_dtype == BF16 and net.deqdss._bw_solver.history_dtype == BF16
    print(f"bf16 training step: forward lowest {net.deqdss.last_forward['lowest']:.2e}, "
          f"backward lowest {net.deqdss.last_backward['lowest']:.2e}")
    got = {k: p.grad for k, p in net.named_parameters()}
    want = {k: torch.from_numpy(T[f"{name}/0/{k}"]) for k in got}
    scale = max(float(t.norm()) for t in want.values())
    for k, w in want.items():
        e = float((got[k].detach().cpu().double() - w.double()).norm()) / max(float(w.double().norm()), 1e-4 * scale)
        assert e < 1e-2, (k, e)


# ---------------------------------------------------------------------------------------------------------- bits, pooling
def _create_opts(eng, plan, threshold, history):
    """A DeviceBroyden whose handle comes from psignn_broyden_create_opts."""
    nat = pkg("_native")
    sv = eng.DeviceBroyden.__new__(eng.DeviceBroyden)
    sv.plan, sv.threshold, sv.keep_trace, sv.device, sv.M = plan, threshold, False, plan.device, plan.N * 10
    sv.history_dtype = BF16 if history else torch.float32
    h = C.c_void_p()
    with torch.cuda.device(plan.device):
        nat.check(nat.lib().psignn_broyden_create_opts(C.byref(h), plan.handle, 0, 0, threshold, 0, 0, history), "create_opts")
    sv.handle = h
    sv._fin = weakref.finalize(sv, nat.lib().psignn_broyden_destroy, h)
    return sv


def test_bf16_history_reproducible_and_separate(dev):
    """Two bf16 solves give the same bits; create_opts(history = 0) is the create_for_batch solver bit for bit; a map's pooled
    solver is handed out only to calls of its own history dtype."""
    eng, solver = pkg("engine"), pkg("utilities.solver")
    g, mesh, md, sd, fmap = _bind("hex26_dirichlet_s0", dev)
    a = solver.broyden(fmap, fmap.h0, threshold=300, eps=1e-7, history_dtype=BF16)
    b = solver.broyden(fmap, fmap.h0, threshold=300, eps=1e-7, history_dtype=BF16)
    assert a["rel_trace"] == b["rel_trace"] and torch.equal(a["result"], b["result"]) and a["n_iter"] == b["n_iter"]
    s_ref = eng.DeviceBroyden(plan=fmap.plan, threshold=300, keep_trace=False)
    s_opt = _create_opts(eng, fmap.plan, 300, 0)
    assert s_opt.nbytes == s_ref.nbytes
    r1, r2 = s_ref.solve(fmap, 1e-7), s_opt.solve(fmap, 1e-7)
    assert r1["rel_trace"] == r2["rel_trace"] and r1["abs_trace"] == r2["abs_trace"] and torch.equal(r1["result"], r2["result"])
    s_b = _create_opts(eng, fmap.plan, 300, 1)
    r3 = s_b.solve(fmap, 1e-7)
    assert r3["rel_trace"] == a["rel_trace"] and torch.equal(r3["result"], a["result"])   # the bf16 constructor, as broyden() uses it
    assert r3["rel_trace"] != r1["rel_trace"]
    for s in (s_ref, s_opt, s_b):
        s.close()
    # pooling: the idle solver is keyed on (threshold, history dtype)
    fm = eng.FixedPointMap(fmap.plan, fmap.weights, fmap.h0, fmap.prb)
    seen = []
    orig = fm.borrow_broyden

    def spy(threshold, history_dtype=torch.float32):
        sv = orig(threshold, history_dtype)
        seen.append((history_dtype, sv.history_dtype, sv.nbytes))
        return sv
    fm.borrow_broyden = spy
    for hd in (BF16, torch.float32, BF16, BF16, torch.float32):
        o = solver.broyden(fm, fm.h0, threshold=300, eps=1e-7, history_dtype=hd, keep_trace=False)
        want = a if hd == BF16 else r1
        assert o["rel_trace"] == want["rel_trace"] and torch.equal(o["result"], want["result"]), hd
    assert all(asked == got for asked, got, _ in seen), seen
    assert seen[0][2] < seen[1][2]
    assert fm._idle_broyden.history_dtype == torch.float32


def test_bf16_config_shard_is_solved_mesh_by_mesh(dev, monkeypatch):
    """solve_shard_batched with a bf16 history configuration: the meshes go through the one-by-one path (the batched kernels
    sweep fp32 pairs only), each result bit-identical to that mesh's own bf16 net.deqdss solve."""
    data, batch, eng = pkg("data"), pkg("batch"), pkg("engine")
    sd = load_weights("dirichlet")
    net = pkg("model_psignn").ModelPSIGNN(dict(latent_dim=10, n_layers=1, fw_tol=1e-5, fw_thres=300,
                                               broyden_history_dtype=BF16))
    net.load_state_dict(sd)
    net = net.to(dev).eval()
    meshes = [data.make_hex_problem(n, seed=s) for s, n in enumerate((13, 26, 40))]
    calls = []
    real = eng.broyden_solve_batch
    monkeypatch.setattr(eng, "broyden_solve_batch", lambda *a, **k: calls.append(1) or real(*a, **k))
    bat = batch.solve_shard_batched(net, meshes, dev)
    assert not calls
    with torch.no_grad():
        for (i, u, loss), m in zip(bat, meshes):
            md = m.to(dev)
            o = net.deqdss(net.autoencoder.encoder(md.x), md)
            assert torch.equal(u, net.autoencoder.decoder(o["result"])) and loss["nsteps"] == o["nstep"], i
    # and the same shard with fp32 pairs does take the batched solver
    net32 = pkg("model_psignn").ModelPSIGNN(dict(latent_dim=10, n_layers=1, fw_tol=1e-5, fw_thres=300))
    net32.load_state_dict(sd)
    batch.solve_shard_batched(net32.to(dev).eval(), meshes, dev)
    assert calls
