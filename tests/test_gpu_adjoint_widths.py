"""GPU: the adjoint solves (Broyden ``adjoint_loop``, restarted GMRES, and their lockstep forms) at 16 floats per lane, step by step.

A handle takes the 16-float vector kernels once its own length, or the shard it was sized for, reaches 3 * 2^18 elements
(``shapes::vec_shape``, csrc/solver_shapes.h).  The other adjoint tests stay below that, so the VEC = 16 instantiations of ``k_addv``,
``kb_xnext``, ``kb_addv_resid`` (solver.hip), ``k_ag_begin``, ``k_ag_keep`` and their batch forms (krylov.hip), ``k_vjp_lin_batch`` under
a 16-float solver and a ``k_ag_check`` over more than 256 block partials run here only.  The width is selected the way production
selects it: ``shard_elems = 1 << 20`` on the fixtures (M = 5 470 = 14 mod 16: two blocks, a ragged last lane), the handle's own
length on a 105 469-node mesh (M = 1 054 690 = 2 mod 16, 258 blocks).  Every wide case first shows that it left the 4-float shapes:
``nbytes`` of the handle differs from its narrow twin's (the partial buffers have one row per block; ``_broyden_is_wide`` says where
that cannot tell and what stands in its place).

No gate is fitted to the device's output.  Each is one of
* bit-identity with a route that is itself step-checked (the host-driven Broyden solve of y -> J^T y + grad through
  ``psignn_broyden_ext_*``: same ``launch_update``, same ``k_resid`` norm partials, so iterates AND traces are equal bit for bit;
  the single solve on the same handle for the lockstep forms);
* a criterion of tests/recurrences.py (``_check_run``: the Broyden recurrences in float64 from the device's own state, whole vector
  and 4 096-element tail; ``_check_traces``) or of the two adjoint GMRES test modules, unchanged;
* ``e_dev <= 16 e32 + 4 EPS32`` in relative L2 against the float64 restatement of one restart cycle (tests/adjoint_gmres_ref.py),
  e32 being the distance of the same restatement in plain fp32 torch from that truth, measured inside the test.

Lines starting with ADJ16 report e_dev / e32 of the one-cycle comparisons.  On an MI355X, ``result`` at 16 floats per lane (at 4):
hex13_dirichlet lin 2.39e-7 / 2.37e-7 (2.61e-7), direct operator 2.80e-7 / 2.37e-7 (2.91e-7); hex13_mixed stored 3.25e-7 / 3.67e-7
(3.76e-7); hex26_dirichlet 4.12e-7 / 3.00e-7 (4.00e-7); 105 469 nodes 6.20e-7 / 6.30e-7.  ``rel_trace[1]`` / ``abs_trace[1]``: e_dev
9.9e-8 - 1.4e-6 against e32 4.2e-7 - 1.4e-6.  The whole module takes 9 s."""
import functools
import os

import pytest
import torch

import adjoint_gmres_ref as ref
from conftest import load_case, load_weights, pkg
from oracle import psignn_oracle as orc
from recurrences import EPS32, _check_run, _check_traces, _run_recorded
from test_gpu_adjoint_batch import _same as _same_broyden
from test_gpu_adjoint_gmres import LIN_CASES, _bind, _rel_of
from test_gpu_adjoint_gmres_batch import _same as _same_gmres
from test_gpu_plan_limits import TAU, Run

pytestmark = pytest.mark.gpu

K = 48
WIDE = 1 << 20                     # a declared shard past the width switch (3 << 18 elements)
SWITCH = 3 << 18
NBIG, HEXBIG = 105469, 187         # make_hex_problem(187): M = 1 054 690, 258 blocks of 16 floats per lane
KBIG = 12


# ------------------------------------------------------------------------------------------------------------ helpers
def _broyden_is_wide(eng, plan, thr, se):
    """The witness: a Broyden handle of (plan, thr, shard_elems = se) against its 4-float twin, the handle made with shard_elems = 0.
    A handle that is wide by its own length has no such twin, and ``nbytes`` cannot tell there: at 1 054 690 elements a 4-float handle
    (PSIGNN_VEC16_MIN raised) allocates the same bytes, since the wide one runs its sweeps over the same 1 030 4-float blocks and only
    the element-wise kernels (k_begin, k_xnext, k_addv, k_resid) differ.  There the witness is the rule itself -- length at or past the
    compiled-in switch, which tests/test_host_solver_shapes.py pins at 3 << 18, and no knob moving it."""
    if plan.N * 10 >= SWITCH:
        assert os.environ.get("PSIGNN_VEC16_MIN") is None
        return
    wide = eng.DeviceBroyden(plan=plan, threshold=thr, keep_trace=True, shard_elems=se)
    narrow = eng.DeviceBroyden(plan=plan, threshold=thr, keep_trace=True, shard_elems=0)
    a, b = wide.nbytes, narrow.nbytes
    wide.close()
    narrow.close()
    assert a != b, ("the handle did not leave the 4-float shapes", a, b)


def _gmres(M, dev, m, se):
    return pkg("engine").DeviceGmres(M, dev, m, shard_elems=se or None)     # (0: a handle sized for itself)


def _gmres_is_wide(M, dev, m, se):
    """The same witness for a GMRES handle (``psignn_gmres_bytes`` counts one row of dot partials per block).  A handle that is wide
    by its own length: it holds FEWER bytes than a handle of the longest vector still below the switch, though it is longer."""
    wide = _gmres(M, dev, m, se)
    narrow = _gmres(M, dev, m, 0) if M < SWITCH else _gmres(SWITCH - 1, dev, m, 0)
    a, b = wide.nbytes - wide.V.numel() * 4, narrow.nbytes - narrow.V.numel() * 4
    wide.close()
    narrow.close()
    assert (a != b) if M < SWITCH else (a < b), ("the handle did not leave the 4-float shapes", a, b)


def _adjoint_map(fmap, H, g, lin):
    """y -> J^T y + grad in the numbering the device solve runs in (plan order; an untiled plan's is the caller's), as the torch
    expression whose two fp32 operations per element ``k_addv`` / ``kb_addv_resid`` repeat."""
    gp = fmap.to_plan(g)
    if lin is not None:
        return lambda yp: lin.vjp_p(yp) + gp
    if fmap.plan.tiled:
        Hp = fmap.to_plan(H)
        return lambda yp: fmap.vjp_p(Hp, yp) + gp
    return lambda y: fmap.vjp(H, y) + g


def _host_driven(fmap, F, g, se, thr):
    """The recorded host-driven solve of F from y0 = 0 (F(0) = grad bit for bit: what ``k_begin`` receives in ``adjoint_loop``)."""
    rec, sv, out = _run_recorded(pkg("engine"), F, torch.zeros_like(g), plan=fmap.plan, shard_elems=se, back=fmap.from_plan, K=thr)
    rec.fwd = fmap.to_plan
    assert torch.equal(F(fmap.to_plan(rec.X[0])), fmap.to_plan(g))
    return rec, sv, out


def _broyden_adjoint_is_the_host_driven_solve(fmap, H, g, lin, se, thr, its_check, its_equal, label):
    eng = pkg("engine")
    F = _adjoint_map(fmap, H, g, lin)
    rec, hsv, host = _host_driven(fmap, F, g, se, thr)
    _check_run(rec, hsv, its_check, label, K=thr)
    hsv.close()
    for i in range(thr):      # k_xnext: one fp32 addition per element (the recurrences take the iterates as they are)
        assert torch.equal(rec.X[i + 1], rec.X[i] + rec.DX[i]), (label, "x_next", i)
    sv = eng.DeviceBroyden(plan=fmap.plan, threshold=thr, keep_trace=True, shard_elems=se)
    out = sv.solve_adjoint(fmap, H, g, 0.0, lin=lin)
    assert out["n_iter"] == thr and out["stop_reason"] == 0, (out["n_iter"], out["stop_reason"])
    for i in its_equal:
        assert torch.equal(sv.iterate(i, g), rec.X[i]), (label, i)
    assert torch.equal(out["result"], sv.iterate(out["nstep"], g)), (label, out["nstep"])
    # both runs form their norm partials in launch_update's k_resid, at the same block shapes: the same bits
    assert out["rel_trace"][:thr] == host["rel_trace"][:thr] and out["abs_trace"][:thr] == host["abs_trace"][:thr], label
    assert out["nstep"] == host["nstep"] and out["lowest"] == host["lowest"]
    # trace entry i belongs to iterate i + 1: abs = |F(x) - x|, rel = abs / (|F(x)| + 1e-9) (check_block, solver.hip)
    P = [rec.X[i + 1].reshape(-1).cpu() for i in range(thr)]
    R = [fmap.from_plan(F(fmap.to_plan(rec.X[i + 1]))).reshape(-1).cpu() for i in range(thr)]
    _check_traces(P, R, list(range(thr)), out["abs_trace"][:thr], out["rel_trace"][:thr], 1e-9, label)
    sv.close()


def _rel(a, truth):
    a, truth = torch.as_tensor(a, dtype=torch.float64).reshape(-1).cpu(), torch.as_tensor(truth, dtype=torch.float64).reshape(-1).cpu()
    return float((a - truth).norm() / truth.norm())


def _one_cycle_gate(label, out, t64, t32):
    """``out``: the device's solve with budget m + 2; t64 / t32: the float64 and the plain-fp32 restatement of the same solve."""
    assert out["n_cycles"] == 2 and out["nstep"] == 11 and out["stop"] == "budget", (label, out["n_cycles"], out["nstep"], out["stop"])
    assert t64["n_cycles"] == 2 and t64["nstep"] == 11 and t64["stop"] == "budget", (label, "truth", t64["stop"])
    assert len(out["rel_trace"]) == 2 and out["lowest"] == out["rel_trace"][1] < out["rel_trace"][0], (label, out["rel_trace"])
    e_dev, e32 = _rel(out["result"], t64["result"]), _rel(t32["result"], t64["result"])
    line = f"ADJ16 {label}: result e_dev {e_dev:.2e} e32 {e32:.2e}"
    gates = [("result", e_dev, e32)]
    for tr in ("rel_trace", "abs_trace"):
        d, p = _rel(out[tr][1], t64[tr][1]), _rel(t32[tr][1], t64[tr][1])
        line += f" | {tr}[1] {out[tr][1]:.6e} (float64 {t64[tr][1]:.6e}) e_dev {d:.2e} e32 {p:.2e}"
        gates.append((tr, d, p))
    print(line)
    for what, d, p in gates:
        assert d <= 16 * p + 4 * EPS32, (label, what, d, p)


# --------------------------------------------------------------- 1. Broyden adjoint = host-driven solve of y -> J^T y + grad
# (fixture, n_layers, tile_target, lin, shard_elems)
BROYDEN_CASES = [("hex13_dirichlet_s0", 1, 0, "direct", 0),            # control: the criterion at the width the suite already trusts
                 ("hex13_dirichlet_s0", 1, 0, "direct", WIDE),         # (dirichlet: the handle's ``neumann`` is ignored)
                 ("hex13_mixed_s1", 1, 0, "stored", WIDE),
                 ("hex13_mixed_s1", 1, 0, "direct", WIDE),
                 ("hex13_dirichlet_s0", 1, 0, None, WIDE),             # direct operator, tiled plan: psignn_f_vjp_p
                 ("hex13_dirichlet_s0", 1, -1, None, WIDE),            # untiled plan: psignn_f_vjp, caller's numbering
                 ("hex13_dirichlet_s0", 2, 0, None, WIDE)]             # two-layer stacked checkpoint: psignn_f_layers_vjp


@pytest.mark.parametrize("name,L,tt,lin,se", BROYDEN_CASES)
def test_broyden_adjoint_is_the_host_driven_solve(name, L, tt, lin, se, dev):
    """``adjoint_loop`` (k_xnext, the transposed product, k_addv, launch_update) against ``solve_callable`` of the same map on a
    solver of the same plan and ``shard_elems``, 48 iterations at eps = 0: every iterate and both traces bit-identical, which carries
    the float64 recurrence check of the host-driven run over to the device loop.  M = 5 470: at 16 floats per lane two blocks, the
    second partial, its last lane ragged."""
    P, fmap, H, g, handle = _bind(name, L, tt, lin, dev)
    if se:
        _broyden_is_wide(pkg("engine"), fmap.plan, K, se)
    _broyden_adjoint_is_the_host_driven_solve(fmap, H, g, handle, se, K, (0, 1, 5, 24, 25, 26, 46), (1, 24, 25, 26, 40, K),
                                              f"{name} L={L} tt={tt} lin={lin} shard={se}")
    if handle is not None:
        handle.close()


# ------------------------------------------------------------------------------------- ragged shard of three small meshes
@functools.lru_cache(maxsize=None)
def _wide_shard():
    """Three hex meshes of different sizes (built as test_gpu_adjoint_batch._shard builds its shards; computed once, left unchanged):
    maps, H* from the lockstep forward solve at 1e-5 / 300, a seeded Gaussian grad and a linearisation at H* per mesh."""
    data, eng = pkg("data"), pkg("engine")
    dev = torch.device("cuda:0")
    sd = load_weights("dirichlet")
    net = pkg("model_psignn").ModelPSIGNN(dict(latent_dim=10, n_layers=1, fw_tol=1e-5, fw_thres=300))
    net.load_state_dict(sd)
    net = net.to(dev).eval()
    mds = [data.make_hex_problem(n, seed=s).to(dev) for s, n in enumerate((13, 26, 10))]
    with torch.no_grad():
        fmaps = [net.deqdss.f.bind(net.autoencoder.encoder(md.x), md) for md in mds]
    assert all(f.plan.tiled for f in fmaps) and len({f.plan.N for f in fmaps}) == 3
    total = sum(f.plan.N for f in fmaps) * 10
    assert total < SWITCH
    fw = [eng.DeviceBroyden(plan=f.plan, threshold=300, keep_trace=False, shard_elems=total) for f in fmaps]
    H = [o["result"] for o in eng.broyden_solve_batch(fw, fmaps, 1e-5)]
    for sv in fw:
        sv.close()
    grads = [torch.randn(h.shape, generator=torch.Generator().manual_seed(100 + i)).to(dev) for i, h in enumerate(H)]
    lins = [f.linearize_p(f.to_plan(h)) for f, h in zip(fmaps, H)]
    return dict(fmaps=fmaps, H=H, grads=grads, lins=lins, total=total)


# ----------------------------------------------------------------------------------------- 2. lockstep Broyden adjoint
def test_lockstep_broyden_adjoint_at_16_floats(dev):
    """``psignn_broyden_solve_adjoint_lin_batch`` with solvers sized for a 2^20-element shard: kb_xnext<16>, k_vjp_lin_batch under a
    16-float solver, kb_addv_resid<16>.  Every mesh, all fields and bits, against the single solve on the same solver object (pinned by
    test_broyden_adjoint_is_the_host_driven_solve: handles of the same shape), at eps = 1e-6 for two poll intervals and at eps = 0, where
    all 48 iterations run and the update chain reaches its window regime under the adjoint head."""
    eng, nat = pkg("engine"), pkg("_native")
    S = _wide_shard()
    for f in S["fmaps"]:
        _broyden_is_wide(eng, f.plan, K, WIDE)
    solvers = [eng.DeviceBroyden(plan=f.plan, threshold=K, keep_trace=False, shard_elems=WIDE) for f in S["fmaps"]]
    assert eng.adjoint_batchable(solvers, S["lins"])
    for eps in (1e-6, 0.0):
        single = [sv.solve_adjoint(f, h, g, eps, lin=l) for sv, f, h, g, l in zip(solvers, S["fmaps"], S["H"], S["grads"], S["lins"])]
        for poll in (8, 3):
            nat.prof_enable(True)
            nat.prof_collect()
            outs = eng.broyden_solve_adjoint_batch(solvers, S["lins"], S["grads"], eps, poll_every=poll)
            ran = nat.prof_collect()
            nat.prof_enable(False)
            for a, b in zip(single, outs):
                _same_broyden(a, b)
            # one product, one x_next and one residual launch per lockstep iteration
            assert "k_vjp_lin" not in ran and "k_addv" not in ran, sorted(ran)
            its = max(o["n_iter"] for o in outs)
            assert ran["k_vjp_lin_batch"][0] == ran["k_xnext"][0] == ran["k_addv_resid"][0] >= its, (eps, poll, ran)
            if eps == 0.0:
                assert its == K and ran["k_vjp_lin_batch"][0] == K and all(o["n_iter"] == K for o in outs)
    for sv in solvers:
        sv.close()


# --------------------------------------------------------------------------------------------------- 3. GMRES adjoint
ONE_CYCLE = [("hex13_dirichlet_s0", "direct"), ("hex13_mixed_s1", "stored"), ("hex26_dirichlet_s0", "direct"), ("hex13_dirichlet_s0", None)]


@pytest.mark.parametrize("se", [0, WIDE])
@pytest.mark.parametrize("name,lin", ONE_CYCLE)
def test_gmres_adjoint_one_restart_cycle_against_float64(name, lin, se, dev):
    """m = 10, budget m + 2: the head of cycle 0, ten Arnoldi steps, the head of cycle 1, then the budget stop -- ``result`` is the
    iterate after one cycle.  Against ``gmres_adjoint`` in float64 on the float64 oracle VJP; the yardstick e32 is the same restatement
    in plain fp32 torch on the CPU.  (On a CPU the restatement gives rel_trace[1] = 4.6e-3 / 9.8e-3 / 8.6e-3 on hex13_dirichlet,
    hex13_mixed, hex26_dirichlet and e32 = 2.0e-7 / 5.2e-7 / 3.6e-7; a wrong width instantiation is off by 1e-2 or more.)
    shard_elems 0: the control at the width the suite already trusts."""
    P, fmap, H, g, handle = _bind(name, 1, 0, lin, dev)
    M = fmap.plan.N * 10
    if se:
        _gmres_is_wide(M, dev, 10, se)
    sv = _gmres(M, dev, 10, se)
    out = sv.solve_adjoint(fmap, H, g, 1e-8, 12, lin=handle)
    t64 = ref.gmres_adjoint(P.vjp64, P.grad.double(), 1e-8, 12, m=10)
    t32 = ref.gmres_adjoint(P.vjp32, P.grad, 1e-8, 12, m=10)
    _one_cycle_gate(f"{name} lin={lin} shard={se}", out, t64, t32)
    sv.close()
    if handle is not None:
        handle.close()


@pytest.mark.parametrize("name,L,tt,lin", [LIN_CASES[0], LIN_CASES[3]])
def test_gmres_whole_solves_at_16_floats(name, L, tt, lin, dev):
    """The gates of test_gpu_adjoint_gmres.test_error_and_products_against_the_broyden_route, unchanged, with both handles made with
    shard_elems = 2^20: only the kernels' width differs from that test."""
    eng = pkg("engine")
    P, fmap, H, g, handle = _bind(name, L, tt, lin, dev)
    M = fmap.plan.N * 10
    _broyden_is_wide(eng, fmap.plan, 500, WIDE)
    _gmres_is_wide(M, dev, 50, WIDE)
    bro_sv = eng.DeviceBroyden(plan=fmap.plan, threshold=500, keep_trace=False, shard_elems=WIDE)
    bro = bro_sv.solve_adjoint(fmap, H, g, 1e-8, lin=handle)
    gm_sv = _gmres(M, dev, 50, WIDE)
    out = gm_sv.solve_adjoint(fmap, H, g, 1e-8, 500, lin=handle)
    e_gm, e_br = P.error(out["result"]), P.error(bro["result"])
    print(f"ADJ16 whole solve {name} lin={lin}: GMRES(50) products {out['nstep']} stop {out['stop']} error {e_gm:.3e} | Broyden products "
          f"{bro['n_iter']} error {e_br:.3e}")
    assert bool(torch.isfinite(out["result"]).all())
    assert e_gm <= 2.0 * e_br, (e_gm, e_br)
    assert out["nstep"] <= bro["n_iter"], (out["nstep"], bro["n_iter"])
    rel = _rel_of(fmap, H, g, handle, out["result"])
    assert abs(rel - out["lowest"]) <= 1e-4 * rel, (rel, out["lowest"])
    assert len(out["rel_trace"]) == len(out["abs_trace"]) == out["n_cycles"] and out["lowest"] == min(out["rel_trace"])
    assert out["rel_trace"][0] == pytest.approx(1.0, abs=1e-6)
    for o in (bro_sv, gm_sv, handle):
        o.close()


def test_lockstep_gmres_adjoint_at_16_floats(dev):
    """``psignn_gmres_solve_adjoint_lin_batch`` with handles sized for a 2^20-element shard (the batch forms of k_ag_begin / k_ag_keep and
    of the Arnoldi kernels at VEC = 16): every replica bit-identical to ``solve_adjoint(..., lin=)`` on the same handle, whatever
    ``poll_every``."""
    eng = pkg("engine")
    S = _wide_shard()
    for f in S["fmaps"]:
        _gmres_is_wide(f.plan.N * 10, dev, 50, WIDE)
    handles = [_gmres(f.plan.N * 10, dev, 50, WIDE) for f in S["fmaps"]]
    assert eng.gmres_adjoint_batchable(handles, S["lins"])
    single = [sv.solve_adjoint(f, h, g, 1e-8, 500, lin=l) for sv, f, h, g, l in zip(handles, S["fmaps"], S["H"], S["grads"], S["lins"])]
    for poll in (8, 3):
        outs = eng.gmres_solve_adjoint_batch(handles, S["lins"], S["grads"], 1e-8, 500, poll_every=poll)
        for r, (a, b) in enumerate(zip(single, outs)):
            _same_gmres(a, b, f"replica {r} poll {poll}")
    assert all(o["nstep"] > 0 and bool(torch.isfinite(o["result"]).all()) for o in single)
    for sv in handles:
        sv.close()


# --------------------------------------------------------------------------------- 4. one natural-size mesh: 105 469 nodes
class _Big:
    """make_hex_problem(187) in the dirichlet family on its default plan; H two f steps from the encoder state (as
    test_gpu_gradients_at_scale.Scale: the linearisation at any state is a valid linear system, nothing here needs convergence), the
    stored linearisation there, a seeded Gaussian grad."""

    def __init__(self, seed, dev, weights=None):
        data, eng = pkg("data"), pkg("engine")
        self.m = data.make_hex_problem(HEXBIG, seed=seed, compute_sol=False)
        assert self.m.num_nodes == NBIG
        self.md = md = self.m.to(dev)
        self.sd = load_weights("dirichlet")
        self.w = eng.PackedWeights(self.sd, dev) if weights is None else weights
        self.plan = eng.MeshPlan(md)
        assert self.plan.tiled
        pre = "autoencoder.encoder.mlp.mlp."
        self.h0 = eng.mlp2(md.x, *[self.sd[pre + k].to(dev) for k in ("0.weight", "0.bias", "2.weight", "2.bias")])
        self.fm = eng.FixedPointMap(self.plan, self.w, self.h0, md.prb_data)
        self.H = self.fm(self.fm(self.h0))
        self.lin = self.fm.linearize_p(self.fm.to_plan(self.H))
        self.g = torch.randn(NBIG, 10, generator=torch.Generator().manual_seed(7 + seed)).to(dev)
        self.M = NBIG * 10


@pytest.fixture(scope="module")
def big(dev):
    cache = {}

    def get(seed):
        if seed not in cache:    # (one packed weight buffer for all meshes: the lockstep solves ask for it)
            cache[seed] = _Big(seed, dev, weights=get(0).w if seed else None)
        return cache[seed]
    yield get
    for b in cache.values():
        b.lin.close()


def test_broyden_adjoint_on_105469_nodes(big, dev):
    """M = 1 054 690 = 2 (mod 16): 16 floats per lane by the handle's own length, 258 blocks, a ragged last lane without any declared
    shard.  12 iterations at eps = 0: iterates and traces bit-identical to the host-driven run, which satisfies the recurrences on the
    whole vector and on the last 4 096 elements.  No outcome gate: the fp32 adjoint solves stall at this size."""
    B = big(0)
    assert B.M >= SWITCH and B.M % 16 == 2 and -(-B.M // 4096) == 258
    _broyden_is_wide(pkg("engine"), B.plan, KBIG, 0)
    _broyden_adjoint_is_the_host_driven_solve(B.fm, B.H, B.g, B.lin, 0, KBIG, (0, 3, 10), (1, 6, KBIG), "105469 nodes")


def test_gmres_adjoint_on_105469_nodes(big, dev):
    """``k_ag_check`` and the Arnoldi reductions over 258 block partials (``block_sum_partials`` takes a second round over its 256
    threads).  One restart cycle against the float64 restatement running ON THE DEVICE with ``FixedPointMap64.vjp`` as its operator;
    the yardstick is the fp32 restatement in plain torch with the device's own transposed product (``lin.vjp_p`` between the plan
    permutations -- gated against float64 at 1M nodes in test_gpu_gradients_at_scale.py, not the code under test here)."""
    eng = pkg("engine")
    B = big(0)
    fm = B.fm
    _gmres_is_wide(B.M, dev, 10, 0)
    sv = _gmres(B.M, dev, 10, 0)
    out = sv.solve_adjoint(fm, B.H, B.g, 1e-8, 12, lin=B.lin)
    rel = _rel_of(fm, B.H, B.g, B.lin, out["result"])
    assert abs(rel - out["lowest"]) <= 1e-4 * rel, (rel, out["lowest"])
    fm64 = eng.FixedPointMap64(B.plan, eng.PackedWeights64(B.sd, dev), B.h0, B.md.prb_data, B.md.edge_attr)
    op32 = lambda v: fm.from_plan(B.lin.vjp_p(fm.to_plan(v)))
    op64 = lambda v: fm64.vjp(B.H, v)
    t32 = ref.gmres_adjoint(op32, B.g, 1e-8, 12, m=10, device=dev)
    t64 = ref.gmres_adjoint(op64, B.g.double(), 1e-8, 12, m=10, device=dev)
    fm64.close()
    _one_cycle_gate("105469 nodes lin", out, t64, t32)
    sv.close()


def test_lockstep_adjoints_on_two_105469_node_meshes(big, dev):
    """Two meshes of this size (seeds 0 and 1), handles at their natural width made with ``shard_elems`` = the shard's total: the
    lockstep Broyden (12 iterations, eps = 0) and GMRES (m = 10, budget 12) adjoint solves, per mesh bit-identical to the single solves
    on the same handles."""
    eng = pkg("engine")
    Bs = [big(0), big(1)]
    total = sum(b.M for b in Bs)
    lins, grads = [b.lin for b in Bs], [b.g for b in Bs]
    for b in Bs:
        _broyden_is_wide(eng, b.plan, KBIG, total)
        _gmres_is_wide(b.M, dev, 10, total)
    solvers = [eng.DeviceBroyden(plan=b.plan, threshold=KBIG, keep_trace=False, shard_elems=total) for b in Bs]
    assert eng.adjoint_batchable(solvers, lins)
    single = [sv.solve_adjoint(b.fm, b.H, b.g, 0.0, lin=b.lin) for sv, b in zip(solvers, Bs)]
    outs = eng.broyden_solve_adjoint_batch(solvers, lins, grads, 0.0)
    for a, o in zip(single, outs):
        assert bool(torch.isfinite(o["result"]).all()) and o["n_iter"] == KBIG
        _same_broyden(a, o)
    for sv in solvers:
        sv.close()
    handles = [_gmres(b.M, dev, 10, total) for b in Bs]
    assert eng.gmres_adjoint_batchable(handles, lins)
    single = [sv.solve_adjoint(b.fm, b.H, b.g, 1e-8, 12, lin=b.lin) for sv, b in zip(handles, Bs)]
    outs = eng.gmres_solve_adjoint_batch(handles, lins, grads, 1e-8, 12)
    for r, (a, o) in enumerate(zip(single, outs)):
        assert bool(torch.isfinite(o["result"]).all()) and o["nstep"] == 11
        _same_gmres(a, o, f"mesh {r}")
    for sv in handles:
        sv.close()


# ------------------------------------------------------------------- 5. the adjoint lockstep on a shard holding a limit tile
@pytest.mark.parametrize("case,mixed,fixture,rows", [("halo512", False, "hex13_dirichlet_s0", 768), ("jvp682", True, "hex13_mixed_s1", 682)])
def test_lockstep_adjoints_with_a_limit_tile(case, mixed, fixture, rows, dev):
    """The counterpart of test_gpu_plan_limits.test_batched_broyden_with_a_768_row_mesh: ``k_vjp_lin_batch`` sizes its LDS by the
    shard's ``max_rows``.  A plan at the row limit of its family plus a fixture mesh: the lockstep Broyden and GMRES adjoint solves per
    mesh bit-identical to the single solves on the same handles; and the limit mesh's stored transposed product against the float64
    oracle, tile by tile, under the gate test_every_kernel_at_the_plan_limits applies."""
    eng = pkg("engine")
    r = Run(case, mixed, dev)
    gold, mesh = load_case(fixture)
    md = mesh.to(dev)
    fm1 = r.fm
    fm2 = eng.FixedPointMap(eng.MeshPlan(md), r.w, torch.from_numpy(gold["h0"]).to(dev), md.prb_data, getattr(md, "unit_normal_vector", None))
    assert fm1.plan.tiled and fm1.plan.max_tile_rows == rows and fm2.plan.max_tile_rows < rows
    neumann = "stored" if mixed else None
    lins = [fm1.linearize_p(fm1.to_plan(r.dev_(r.h)), neumann=neumann), fm2.linearize_p(fm2.to_plan(fm2.h0), neumann=neumann)]
    fmaps, states = [fm1, fm2], [r.dev_(r.h), fm2.h0]
    grads = [torch.randn(f.plan.N, 10, generator=torch.Generator().manual_seed(300 + i)).to(dev) for i, f in enumerate(fmaps)]
    total = sum(f.plan.N for f in fmaps) * 10
    solvers = [eng.DeviceBroyden(plan=f.plan, threshold=8, keep_trace=False, shard_elems=total) for f in fmaps]
    handles = [_gmres(f.plan.N * 10, dev, 6, total) for f in fmaps]
    try:
        assert eng.adjoint_batchable(solvers, lins) and eng.gmres_adjoint_batchable(handles, lins)
        single = [sv.solve_adjoint(f, h, g, 0.0, lin=l) for sv, f, h, g, l in zip(solvers, fmaps, states, grads, lins)]
        outs = eng.broyden_solve_adjoint_batch(solvers, lins, grads, 0.0)
        for a, b in zip(single, outs):
            assert bool(torch.isfinite(a["result"]).all()) and bool(torch.isfinite(b["result"]).all())
            _same_broyden(a, b)
        single = [sv.solve_adjoint(f, h, g, 0.0, 8, lin=l) for sv, f, h, g, l in zip(handles, fmaps, states, grads, lins)]
        outs = eng.gmres_solve_adjoint_batch(handles, lins, grads, 0.0, 8)
        for i, (a, b) in enumerate(zip(single, outs)):
            assert bool(torch.isfinite(a["result"]).all()) and bool(torch.isfinite(b["result"]).all())
            _same_gmres(a, b, f"mesh {i}")
        want = orc.function_vjp(r.s64, r.h.double(), r.h0.double(), r.m64, r.wv.double())
        want32 = orc.function_vjp(r.sd, r.h, r.h0, r.m, r.wv)
        r.check("lin.vjp_p beside the lockstep solves", fm1.from_plan(lins[0].vjp_p(fm1.to_plan(r.dev_(r.wv)))), want, want32, TAU["vjp"])
    finally:
        for o in solvers + handles + lins:
            o.close()
