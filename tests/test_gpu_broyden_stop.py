"""GPU: the stop decision and the kept iterate of every device Broyden solver against ``broyden_stop_ref.replay``.

The update of the Broyden solvers is pinned elsewhere (test_gpu_solver_forms.py, test_gpu_adjoint_widths.py); those tests run to the
threshold on purpose.  Here: when the solve stops, why, and which iterate it returns.  The device keeps its traces as doubles and
decides in doubles (``check_block`` in csrc/solver.hip for every fp32 solver, ``k_b64_test`` in csrc/solver_f64.hip), so every
figure a solve reports must EQUAL the reference's rules replayed over the solve's own traces: n_iter, stop_reason, prot_break,
lowest, nstep and both padded traces, with no tolerance.  Trajectories are chaotic in their tails, so the judge is always the replay
of the device's own trace, never a CPU trajectory.  ``replay`` itself is pinned to the CPU oracle by test_host_broyden_stop.py.

a. Scripted maps through ``utilities.solver.broyden(callable, ...)`` (``psignn_broyden_ext_*``): every case of
   ``broyden_stop_ref.CASES`` -- all four reasons, the off-by-one edges of the stagnation rule, the lowest iterate several steps
   back, the width in the break's limit -- with fp32 and bf16 history, both stop modes, iterates kept and not kept (the buffer
   rotation cur / low / nxt of ``check_block``): the case's reason at the case's step, ``result`` bit-equal to the x handed to call
   ``nstep``, and the two rotations bit-equal to each other.  On one block, on (409, 10), at width 7, and on the three vector
   lengths of test_library_runs_the_recorded_schedule, where ``check_block`` runs inside ``k_reduce_check``, ``k_reduce_a_check``
   and the 16-floats-per-lane forms.
b. Natural maps: the fused single solve, both adjoint solves, a ragged shard forward and adjoint.
c. Float64: ``DeviceBroyden64.solve`` and ``.solve_adjoint``; no float64 iterate is exposed, so ``result`` is checked to be the
   iterate of step ``nstep`` by a second solve with ``threshold = nstep``, which must return the same bits.

Natural stops (parts b and c).  Each natural solve was run once on the MI355X to threshold 300 with no tolerance (eps 0: the
iterates do not depend on eps, so this is the trace of every eps up to its stop) and the trace replayed over a scan of eps
(scripts/broyden_stop_cases.py; profiles/broyden_stop_cases.json holds the traces' summary and the scan).  The note above ``NATURAL``
quotes what was chosen per solver and names the solvers in which no eps gives a natural stagnation stop or break.

Tried in scratch builds of ``check_block``, not kept, against the (16, 10) fp32 cases: ``n >= 30`` for ``n > 30`` (stagnation_at_31
stops at step 30, "stopped at a step where no rule fires"), a window of 29 entries (window_is_30 stops at 39, the same message),
and ``low`` not updated in the rotation (already tolerance_at_5, the first case run: "result is not iterate nstep" when the iterates
are not kept).  Each fails in both stop modes."""
import json
import os

import pytest
import torch

import broyden_stop_ref as bsr
from conftest import CASES, GOLDEN, load_case, load_weights, pkg
from oracle import psignn_oracle as orc

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
_KNOBS = ("PSIGNN_U2D_FORM", "PSIGNN_U2D_KEEP", "PSIGNN_U2D_KMAX", "PSIGNN_UVU", "PSIGNN_JGROUPS", "PSIGNN_VEC16_MIN", "PSIGNN_VEC_AX4")
FIELDS = ("n_iter", "nstep", "stop_reason", "prot_break")


def _same_solve(a, b, what):
    """Two solves that may differ only in where they keep their buffers: counts, traces and result bit for bit."""
    for k in FIELDS:
        assert a[k] == b[k], (what, k, a[k], b[k])
    assert bsr._same_doubles([a["lowest"]], [b["lowest"]]), (what, "lowest")
    assert bsr._same_doubles(a["rel_trace"], b["rel_trace"]) and bsr._same_doubles(a["abs_trace"], b["abs_trace"]), (what, "traces")
    assert torch.equal(a["result"], b["result"]), (what, "result")


# ====================================================================================================== a. scripted, ext route
def _ext(stop_mode, hist, keep_trace):
    solver = pkg("utilities.solver")

    def solve(f, x0, threshold, eps):
        return solver.broyden(f, x0, threshold=threshold, eps=eps, stop_mode=stop_mode, keep_trace=keep_trace, history_dtype=hist)
    return solve


def _scripted(cases, x0, stop_mode, hist, label):
    seen = set()
    for case in cases:
        on, sc_on, rp = bsr.run_case(case, _ext(stop_mode, hist, True), x0, stop_mode)
        off, sc_off, _ = bsr.run_case(case, _ext(stop_mode, hist, False), x0, stop_mode)
        _same_solve(on, off, (label, case.name))
        # the kept iterates are the x the map was handed, the result is one of them
        n, k = on["n_iter"], on["nstep"]
        assert len(on["xest_trace"]) == n + 1 and torch.equal(on["xest_trace"][k], on["result"]), (label, case.name)
        for i in {1, k, n}:
            assert torch.equal(on["xest_trace"][i], sc_on.xs[i]), (label, case.name, i)
        assert sc_on.calls == sc_off.calls and torch.equal(sc_on.xs[k], sc_off.xs[k]), (label, case.name)
        print(f"STOP ext {label} {stop_mode} {case.name}: {bsr.REASONS[on['stop_reason']]} ({on['stop_reason']}) at step {n}, lowest at {k}")
        seen.add(on["stop_reason"])
    return seen


@pytest.mark.parametrize("stop_mode", ["rel", "abs"])
@pytest.mark.parametrize("hist", [torch.float32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", [(16, 10), (409, 10), (16, 7)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_scripted_stops_on_the_ext_route(shape, hist, stop_mode, dev, monkeypatch):
    """Every case of the table on one block (160 elements), on (409, 10) and at width 7 (where the two seq_len cases run)."""
    for k in _KNOBS:
        monkeypatch.delenv(k, raising=False)
    x0 = bsr.start_vector(shape, device=dev)
    label = f"{shape[0]}x{shape[1]} {'bf16' if hist == BF16 else 'fp32'}"
    seen = _scripted(bsr.cases_for(shape[1], stop_mode), x0, stop_mode, hist, label)
    assert seen == {0, 1, 2, 3}, seen


def test_seq_len_reaches_the_kernel(dev):
    """One script, two widths: 9e-2 at step 5 is past the limit rel_1 * 1e3 * 7 = 0.07 and not past rel_1 * 1e3 * 10 = 0.1."""
    for d, name in ((7, "seq_len_7_breaks"), (10, "seq_len_10_does_not")):
        x0 = bsr.start_vector((16, d), device=dev)
        out, _, _ = bsr.run_case(bsr.CASE[name], _ext("rel", torch.float32, None), x0, "rel")
        assert out["prot_break"] == (d == 7)


@pytest.fixture(scope="module")
def schedule_table():
    with open(os.path.join(GOLDEN, "broyden_schedule.json")) as f:
        return {r["case"]: r for r in json.load(f)}


@pytest.mark.parametrize("stop_mode", ["rel", "abs"])
@pytest.mark.parametrize("hist", [torch.float32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("row", ["m4090", "width_switch", "above_reg_fold"])
def test_scripted_stops_on_the_recorded_shapes(row, hist, stop_mode, schedule_table, dev, monkeypatch):
    """The vector lengths of test_library_runs_the_recorded_schedule, selected as that test selects them (no knob set; (M / 10, 10)
    when 10 divides M, else (M, 1)): M = 4 090 (two-pass form, ``k_reduce_check``), 3 << 18 (the width switch: three sweeps,
    ``k_reduce_a_check``, 16 floats per lane) and 2 047 * 1 024 + 1 (an odd length: the last element starts at 0 and stays there).
    Stagnation at 31, the lowest iterate at step 3 of 35, and the protective break, whose limit follows the width (1 on the long
    vectors)."""
    for k in _KNOBS:
        monkeypatch.delenv(k, raising=False)
    M = schedule_table[row]["M"]
    seq = 10 if M % 10 == 0 else 1
    x0 = bsr.start_vector((M // seq, seq), device=dev)
    label = f"{row} {'bf16' if hist == BF16 else 'fp32'}"
    seen = _scripted([bsr.CASE[n] for n in bsr.LONG_CASES], x0, stop_mode, hist, label)
    assert seen == {2, 3}, seen


# ============================================================================================ b / c. natural maps: the solvers
_cache = {}


def _fmap(name, dev):
    """A fixture's map, or ``hex60``: make_hex_problem(60), 10 981 nodes, trained dirichlet weights, from the encoder state."""
    if name not in _cache:
        eng = pkg("engine")
        if name == "hex60":
            mesh = pkg("data").make_hex_problem(60, seed=0, compute_sol=False)
            assert mesh.num_nodes == 10981
            sd = load_weights("dirichlet")
            with torch.no_grad():
                h0 = orc.encoder(sd, mesh.x)
        else:
            g, mesh = load_case(name)
            sd = load_weights(CASES[name])
            h0 = torch.from_numpy(g["h0"])
        md = mesh.to(dev)
        fmap = eng.FixedPointMap(eng.plan_for(md), eng.PackedWeights(sd, dev), h0.to(dev), md.prb_data, getattr(md, "unit_normal_vector", None))
        _cache[name] = (fmap, md, mesh, sd)
    return _cache[name][0]


class Forward:
    """``DeviceBroyden.solve``: the fused single solve.  ``run`` -> (out, iterate ``nstep`` when the iterates were kept)."""

    def __init__(self, name, stop_mode, dev):
        self.fmap, self.stop_mode = _fmap(name, dev), stop_mode

    def run(self, eps, threshold, keep_trace):
        sv = pkg("engine").DeviceBroyden(plan=self.fmap.plan, threshold=threshold, keep_trace=keep_trace)
        sv.set_stop_mode(self.stop_mode)
        out = self._solve(sv, eps)
        kept = sv.iterate(out["nstep"], out["result"]) if keep_trace else None
        sv.close()
        return out, kept

    def _solve(self, sv, eps):
        return sv.solve(self.fmap, eps)


class Adjoint(Forward):
    """``DeviceBroyden.solve_adjoint`` at the fixed point of the forward solve (eps 1e-5, threshold 300) with a seeded Gaussian
    gradient: ``psignn_broyden_solve_adjoint`` (the VJP kernel in the loop) or, ``lin=True``, ``psignn_broyden_solve_adjoint_lin``."""

    def __init__(self, name, stop_mode, dev, lin):
        super().__init__(name, stop_mode, dev)
        key = ("h*", name)
        if key not in _cache:
            hs = Forward(name, "rel", dev).run(1e-5, 300, False)[0]["result"]
            grad = torch.randn(hs.shape, generator=torch.Generator().manual_seed(9)).to(dev)
            _cache[key] = (hs, grad, self.fmap.linearize_p(self.fmap.to_plan(hs)))
        self.hs, self.grad, l = _cache[key]
        self.lin = l if lin else None

    def _solve(self, sv, eps):
        return sv.solve_adjoint(self.fmap, self.hs, self.grad, eps, lin=self.lin)


class Forward64:
    """``DeviceBroyden64.solve`` from the encoder state / ``.solve_adjoint`` (``adjoint=True``) at that state with a seeded gradient."""
    stop_mode = "rel"

    def __init__(self, name, dev, adjoint=False):
        from test_gpu_f64 import Problem, fixture_problem
        key = ("p64", name)
        if key not in _cache:
            if name == "hex60":
                mesh = pkg("data").make_hex_problem(60, seed=0, compute_sol=False)
                _cache[key] = Problem(mesh, load_weights("dirichlet"), dev)
            else:
                _cache[key] = fixture_problem(name, dev)
        self.p, self.adjoint, self.dev = _cache[key], adjoint, dev
        self.H = self.p.h0.to(dev)
        self.grad = torch.randn(self.H.shape, generator=torch.Generator().manual_seed(9), dtype=torch.float64).to(dev)

    def run(self, eps, threshold, keep_trace=False):
        sv = pkg("engine").DeviceBroyden64(self.p.fmap, threshold)
        out = sv.solve_adjoint(self.H, self.grad, eps) if self.adjoint else sv.solve(self.H, eps)
        sv.close()
        return out, None


def natural(dev):
    """label -> solver object, every natural single solve of parts b and c."""
    out = {}
    for name in ("hex13_dirichlet_s0", "hex13_mixed_s1", "hex60"):
        for mode in ("rel", "abs"):
            out[f"forward/{name}/{mode}"] = lambda name=name, mode=mode: Forward(name, mode, dev)
    for name in ("hex13_dirichlet_s0", "hex60"):
        for mode in ("rel", "abs"):
            out[f"adjoint/{name}/{mode}"] = lambda name=name, mode=mode: Adjoint(name, mode, dev, False)
            out[f"adjoint_lin/{name}/{mode}"] = lambda name=name, mode=mode: Adjoint(name, mode, dev, True)
        out[f"forward64/{name}/rel"] = lambda name=name: Forward64(name, dev)
        out[f"adjoint64/{name}/rel"] = lambda name=name: Forward64(name, dev, adjoint=True)
    return out


SHARD_SIZES = (10, 13, 11, 26, 12, 40)


class Shard:
    """A ragged shard of six dirichlet meshes (the sizes of test_gpu_adjoint_batch.py): ``broyden_solve_batch`` and, at the fixed
    points of that solve at eps 1e-5 / threshold 300, ``broyden_solve_adjoint_batch``; each beside the single solves of the same
    solver objects."""

    def __init__(self, dev):
        data, eng = pkg("data"), pkg("engine")
        sd = load_weights("dirichlet")
        net = pkg("model_psignn").ModelPSIGNN(dict(latent_dim=10, n_layers=1, fw_tol=1e-5, fw_thres=300))
        net.load_state_dict(sd)
        net = net.to(dev).eval()
        self.mds = [data.make_hex_problem(n, seed=s, compute_sol=False).to(dev) for s, n in enumerate(SHARD_SIZES)]
        with torch.no_grad():
            self.fmaps = [net.deqdss.f.bind(net.autoencoder.encoder(md.x), md) for md in self.mds]
        self.total = sum(f.plan.N for f in self.fmaps) * 10
        self.eng = eng
        sv = self.solvers(300, "rel")
        self.H = [o["result"] for o in eng.broyden_solve_batch(sv, self.fmaps, 1e-5)]
        for s in sv:
            s.close()
        self.grads = [torch.randn(h.shape, generator=torch.Generator().manual_seed(100 + i)).to(dev) for i, h in enumerate(self.H)]
        self.lins = [f.linearize_p(f.to_plan(h)) for f, h in zip(self.fmaps, self.H)]

    def solvers(self, threshold, stop_mode):
        sv = [self.eng.DeviceBroyden(plan=f.plan, threshold=threshold, keep_trace=False, shard_elems=self.total) for f in self.fmaps]
        for s in sv:
            s.set_stop_mode(stop_mode)
        return sv

    def run(self, adjoint, eps, threshold, stop_mode="rel"):
        """(batched, single): the per-mesh dictionaries of the lockstep solve and of each mesh alone on the same solver objects."""
        sv = self.solvers(threshold, stop_mode)
        if adjoint:
            single = [s.solve_adjoint(f, h, g, eps, lin=l) for s, f, h, g, l in zip(sv, self.fmaps, self.H, self.grads, self.lins)]
            outs = self.eng.broyden_solve_adjoint_batch(sv, self.lins, self.grads, eps)
        else:
            single = [s.solve(f, eps) for s, f in zip(sv, self.fmaps)]
            outs = self.eng.broyden_solve_batch(sv, self.fmaps, eps)
        for s in sv:
            s.close()
        return outs, single


# ============================================================================================= b / c. natural maps: the tests
# (eps, threshold, the reason the solve ends on).  Measured on the MI355X (profiles/broyden_stop_cases.json; the solves are bitwise
# reproducible): each solve once to threshold 300 with no tolerance, its trace replayed over eps = 10^(k/8).
#   * natural STAGNATION exists in the fused forward solve of the two 547-node fixtures, in both stop modes -- rel: eps 2.4e-8 ..
#     4.2e-8 on hex13_dirichlet_s0 (chosen 3.162e-8: stops at step 234, the lowest iterate ten steps back at 224) and 2.4e-8 .. 5.6e-8
#     on hex13_mixed_s1 (chosen 4.217e-8: step 283, lowest at 274); abs: 1e-6 and 1.778e-6, the same steps -- and in four of the six
#     meshes of the forward shard (rel 3.162e-8: steps 187 / 229 / 176 / 213; abs 1e-6: the same steps).
#   * NO eps gives a natural stagnation stop in: the forward solve of the 10 981-node mesh (its tail moves by a factor 79 within 30
#     steps), any fp32 adjoint solve, single or in the shard (tail ratios 1.5 .. 630), and any float64 solve (tail ratios 10 .. 640:
#     float64 solves keep falling, or rattle at 1e-16).  Reason 2 of those fp32 solvers is covered through the ``check_block`` they
#     share with the scripted cases of part a and with the forward solves here; reason 2 of ``k_b64_test`` (float64) is NOT covered
#     by any test.
#   * NO natural protective break occurs within 300 steps in any of these solves; the one natural break the suite knows is the
#     bf16-history solve of hex13_mixed_s1 at step 250 (test_gpu_broyden_bf16.py), replayed below.  Float64: reason 3 not covered.
_FIX13, _BIG = (1e-5, 300, 1), (1e-5, 300, 0)
_THR = (1e-12, 40, 0)
NATURAL = {
    "forward/hex13_dirichlet_s0/rel": [_FIX13, _THR, (3.162e-8, 300, 2)],
    "forward/hex13_dirichlet_s0/abs": [_FIX13, _THR, (1e-6, 300, 2)],
    "forward/hex13_mixed_s1/rel": [_FIX13, _THR, (4.217e-8, 300, 2)],
    "forward/hex13_mixed_s1/abs": [_FIX13, _THR, (1.778e-6, 300, 2)],
    "forward/hex60/rel": [_BIG, _THR], "forward/hex60/abs": [_BIG, _THR],
    "adjoint/hex13_dirichlet_s0/rel": [_FIX13, _THR], "adjoint/hex13_dirichlet_s0/abs": [_FIX13, _THR],
    "adjoint_lin/hex13_dirichlet_s0/rel": [_FIX13, _THR], "adjoint_lin/hex13_dirichlet_s0/abs": [_FIX13, _THR],
    "adjoint/hex60/rel": [_BIG, _THR], "adjoint/hex60/abs": [_BIG, _THR],
    "adjoint_lin/hex60/rel": [_BIG, _THR], "adjoint_lin/hex60/abs": [_BIG, _THR],
}
NATURAL64 = {
    "forward64/hex13_dirichlet_s0/rel": [(1e-11, 300, 1), (1e-14, 40, 0)],
    "adjoint64/hex13_dirichlet_s0/rel": [(1e-11, 300, 1), (1e-14, 40, 0)],
    "forward64/hex60/rel": [(1e-11, 300, 0), (1e-14, 40, 0)],
    "adjoint64/hex60/rel": [(1e-11, 300, 0), (1e-14, 40, 0), (1e-6, 300, 1)],
}


@pytest.mark.parametrize("label", list(NATURAL))
def test_natural_single_solves(label, dev):
    """``DeviceBroyden.solve`` / ``.solve_adjoint`` (direct and through the stored linearisation): everything reported equals the
    replay; the solve that does not keep its iterates (rotation over three buffers) equals the one that does, bit for bit; the result
    is iterate ``nstep`` of the kept ones; the reason is the measured one (``NATURAL``)."""
    sv = natural(dev)[label]()
    for eps, thr, reason in NATURAL[label]:
        on, kept = sv.run(eps, thr, True)
        off, _ = sv.run(eps, thr, False)
        what = (label, eps, thr)
        rp = bsr.assert_replay(on, eps, thr, 10, sv.stop_mode, what=label)
        _same_solve(on, off, what)
        assert torch.equal(on["result"], kept), what
        print(f"STOP {label} eps {eps:g} threshold {thr}: {bsr.REASONS[on['stop_reason']]} ({on['stop_reason']}) at step {on['n_iter']}, "
              f"lowest {on['lowest']:.3e} at {on['nstep']}")
        assert rp["stop_reason"] == reason, (what, rp["stop_reason"], on["n_iter"])


@pytest.mark.parametrize("label", list(NATURAL64))
def test_natural_float64_solves(label, dev):
    """``DeviceBroyden64.solve`` / ``.solve_adjoint`` (``k_b64_test``, ``k_b64_keep``): everything reported equals the replay, and
    ``result`` is the iterate of step ``nstep``: a second solve with ``threshold = nstep`` -- which cannot know what follows the kept
    step -- ends there with the same traces and returns the same bits."""
    sv = natural(dev)[label]()
    for eps, thr, reason in NATURAL64[label]:
        out, _ = sv.run(eps, thr)
        what = (label, eps, thr)
        rp = bsr.assert_replay(out, eps, thr, 10, "rel", what=label)
        k = out["nstep"]
        assert 1 <= k <= out["n_iter"]
        short, _ = sv.run(eps, k)
        bsr.assert_replay(short, eps, k, 10, "rel", what=label + " to nstep")
        assert short["n_iter"] == short["nstep"] == k, (what, short["n_iter"], short["nstep"])
        assert bsr._same_doubles(short["rel_trace"][:k], out["rel_trace"][:k]) and bsr._same_doubles(short["abs_trace"][:k], out["abs_trace"][:k]), what
        assert torch.equal(short["result"], out["result"]), (what, "result is not iterate nstep")
        print(f"STOP {label} eps {eps:g} threshold {thr}: {bsr.REASONS[out['stop_reason']]} ({out['stop_reason']}) at step {out['n_iter']}, "
              f"lowest {out['lowest']:.3e} at {k}")
        assert rp["stop_reason"] == reason, (what, rp["stop_reason"], out["n_iter"])


@pytest.fixture(scope="module")
def shard(dev):
    return Shard(dev)


# (adjoint, stop_mode, eps, threshold, the reasons of the six meshes as measured)
SHARD_RUNS = [
    (False, "rel", 1e-6, 300, [1, 1, 1, 1, 1, 0]),
    (False, "rel", 3.162e-8, 300, [2, 2, 2, 0, 2, 0]),
    (False, "abs", 1e-6, 300, [2, 2, 2, 0, 2, 0]),
    (False, "rel", 1e-12, 40, [0] * 6),
    (True, "rel", 1e-6, 300, [1, 1, 1, 1, 1, 0]),
    (True, "abs", 1e-5, 300, [1, 1, 1, 0, 1, 0]),
    (True, "rel", 1e-12, 40, [0] * 6),
]


@pytest.mark.parametrize("adjoint,stop_mode,eps,thr,reasons", SHARD_RUNS,
                         ids=[f"{'adjoint' if a else 'forward'}-{m}-{e:g}-{t}" for a, m, e, t, _ in SHARD_RUNS])
def test_natural_shard_solves(adjoint, stop_mode, eps, thr, reasons, shard):
    """``broyden_solve_batch`` / ``broyden_solve_adjoint_batch`` on a ragged shard (``kb_reduce_check`` / ``kb_reduce_a_check``): the
    meshes end at different steps and for different reasons while the lockstep runs on; each equals its own single solve bit for bit
    and the replay of its own traces."""
    outs, single = shard.run(adjoint, eps, thr, stop_mode)
    for i, (o, s) in enumerate(zip(outs, single)):
        what = ("adjoint" if adjoint else "forward", i, stop_mode, eps, thr)
        bsr.assert_replay(o, eps, thr, 10, stop_mode, what=str(what))
        _same_solve(o, s, what)
    print(f"STOP shard {'adjoint' if adjoint else 'forward'} {stop_mode} eps {eps:g} threshold {thr}: reasons {[o['stop_reason'] for o in outs]} "
          f"at steps {[o['n_iter'] for o in outs]}, lowest at {[o['nstep'] for o in outs]}")
    assert [o["stop_reason"] for o in outs] == reasons
    if thr == 300:
        assert len({o["n_iter"] for o in outs}) >= 4 and set(reasons) != {1}


def test_the_recorded_bf16_break_replays(dev):
    """The one natural protective break the suite knows (test_gpu_broyden_bf16.py: hex13_mixed_s1 with bf16 pairs, eps 1e-7,
    threshold 1 000, ends on reason 3 at step 250 with the lowest iterate at 123): the replay of its traces breaks there too, and the
    result is the kept iterate 123, with and without the kept trace."""
    solver = pkg("utilities.solver")
    fmap = _fmap("hex13_mixed_s1", dev)
    on = solver.broyden(fmap, fmap.h0, threshold=1000, eps=1e-7, history_dtype=BF16, keep_trace=True)
    off = solver.broyden(fmap, fmap.h0, threshold=1000, eps=1e-7, history_dtype=BF16, keep_trace=False)
    rp = bsr.assert_replay(on, 1e-7, 1000, 10, "rel", what="bf16 hex13_mixed_s1")
    _same_solve(on, off, "bf16 hex13_mixed_s1")
    assert torch.equal(on["xest_trace"][on["nstep"]], on["result"])
    print(f"STOP bf16 hex13_mixed_s1: {bsr.REASONS[on['stop_reason']]} at step {on['n_iter']}, lowest at {on['nstep']}")
    assert rp["stop_reason"] == 3 and on["prot_break"] and on["nstep"] < on["n_iter"] - 100
