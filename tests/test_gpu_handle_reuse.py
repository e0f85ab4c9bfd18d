"""GPU: a solver handle carries nothing from one solve into the next.

Training keeps its device solver handles and runs a different solve on them at every step (other weights, another encoder state,
another cotangent, another way to end); the other solver tests make a handle per run or repeat one problem on it, where a value
that leaks from the last solve equals the value a clean handle computes.  Here every handle kind runs solve A, then a solve B that
differs from A in every input its entry point takes, and the same B runs alone on a fresh handle made with the same constructor
arguments.  The two B's must be EQUAL: every field of the two dictionaries (``handle_reuse.same_out``: result, n_iter, nstep,
stop_reason, prot_break, lowest, lowest_abs, both padded traces, low_idx, the cycle traces, products, second passes), tensors and
doubles bit for bit.  Nothing in this module has a tolerance of its own, with one exception that is not a reuse check: the GMRES B
that is held against the float64 restatement goes through ``handle_reuse.gmres_against_restatement``, the suite's existing gate
(tests/test_gpu_adjoint_widths.py::_one_cycle_gate: 16 x the plain-fp32 restatement's own error plus 4 ulp) at another restart length.

Two assertions keep a pair from passing vacuously: A ended the way it was chosen to end (scripted A's: the case's reason and step,
``broyden_stop_ref.run_case``; natural A's: the stop recorded in ``test_gpu_broyden_stop.NATURAL`` and, for the step, in
profiles/broyden_stop_cases.json), and B's first trace entries are not A's (``handle_reuse.Reused.follow``).  One B per handle kind
is also held, on the reused handle, against the independent reference the suite has for that kind -- ``bsr.assert_replay`` (every
Broyden link), ``recurrences.check_anderson`` through a ``Recorder``, the ``adjoint_gmres_ref`` restatement in float64 -- so that
"equal to a fresh handle" cannot mean "both wrong".  Each pair prints one line starting with REUSE.

What is not here: the untiled plan has no stored linearisation (``Linearization`` needs a tiled plan), so its chain has no
``lin=`` link, and ``NATURAL`` records tiled plans only, so its first link is held to the replay of its own trace, not to a
recorded step.  At the width switch M = 3 << 18 is no multiple of 10, so that handle is made flat, with seq_len 1 and a start of shape
(M, 1), as tests/test_gpu_broyden_stop.py selects it; the other plan-less handles have seq_len 10.  The endings of the shard solves
are the ones these deterministic solves have on the MI355X, stated mesh by mesh.

Tried in scratch builds of the library, not kept, one dropped reset each:
  * ``st->lowest_rel = 1e8`` dropped from ``k_init_status`` (csrc/solver.hip): 20 of the module's tests fail, first
    test_scripted_solves_follow_each_other_on_one_handle[fp32-rotation-0] ("(0, 5, 'tolerance_at_5 (16, 10)', 'rel', 0.001, 45)":
    nstep 0 where the replay says 5); the natural chains fail on "'lowest'" of "reused handle against a fresh one".
  * ``st->low = 0`` dropped from ``k_init_status``: passes every pair in which B has a finite first step -- any finite value is below
    1e8, so ``check_block`` assigns ``low`` at step 1 -- and is pinned by test_a_solve_that_finds_no_lowest_iterate_returns_its_start
    alone.  The dropped reset leaves a buffer index unset: on a fresh handle it is whatever the allocation held (the ``Status`` block is
    not cleared when it is made), and that scratch build, run when the test still made its fresh handle first, did not fail but read the
    result out of bounds in ``finish`` ("an illegal memory access was encountered").  The test now judges the reused handle's B before a
    fresh handle exists: there ``low`` is A's index (2 / 1 in the rotation after protective_break / lowest_not_last, 3 with kept
    iterates, by the rotation of ``check_block``), a buffer that the NaN solve never writes, so the regression ends in "result is not
    the start vector".  That order was reasoned from the code, not run against the scratch build again.
  * the ``alpha[]`` reset dropped from ``fp_init_body`` (csrc/fpiter.hip), ``if (k == 0) t.a_ready() = 0;`` dropped from
    ``update_chain`` (csrc/solver_shapes.h), ``lowest`` dropped from ``ag_init_body`` (csrc/krylov.hip): the module passes with each
    of them, and reading the code says it must, as it stands: ``k_and_solve`` writes ``alpha[0 .. n)`` before ``k_and_mix`` reads
    those entries; at k = 0 no ``a_j`` is consumed (kd = 0) and ``a_ready`` is cleared after ``reduce_a_check`` of the same iteration;
    ``ag_check_body`` assigns ``lowest`` in cycle 0 whatever it held (``c == 0 || rel < lowest``).  These three resets are redundant
    today; the pairs here would show the day one of them stops being so."""
import functools
import json
import os

import pytest
import torch

import adjoint_gmres_ref as ref
import broyden_stop_ref as bsr
import handle_reuse as hr
import recurrences as rc
from conftest import CASES, GOLDEN, ROOT, load_case, load_weights, pkg
from test_gpu_broyden_stop import _KNOBS, NATURAL, NATURAL64, _same_solve
from test_gpu_fpiter_batch import _random, _stepwise_anderson, _stepwise_picard

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
DEV = "cuda:0"


def _seeded(shape, seed, scale=1.0, dtype=torch.float32):
    return (scale * torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=dtype)).to(DEV)


# ==================================================================================== 1. scripted maps, one plan-less handle
class _ExtHandle:
    """One plan-less ``DeviceBroyden`` (threshold 45) and fresh ones like it, driven through ``solve_callable``."""

    def __init__(self, shape, hist, keep_trace):
        self.shape, self.hist, self.keep = shape, hist, keep_trace
        self.sv = self.make()

    def make(self):
        return pkg("engine").DeviceBroyden(threshold=45, keep_trace=self.keep, n_elems=self.shape[0] * self.shape[1], seq_len=self.shape[1],
                                           device=torch.device(DEV), history_dtype=self.hist)

    def run(self, sv, case, mode, seed):
        """``case`` on ``sv`` in ``mode`` from ``start_vector(seed)``: ``run_case`` asserts the case's reason and step, the replay of
        the solve's own traces and that ``result`` is the x handed to call ``nstep``."""
        assert case.threshold == 45
        sv.set_stop_mode(mode)
        x0 = bsr.start_vector(self.shape, device=torch.device(DEV), seed=seed)
        out, sc, _ = bsr.run_case(case, lambda f, x, thr, eps: sv.solve_callable(f, x, eps), x0, mode)
        return dict(out, eps=sc.eps(case.eps), x0=x0)

    def fresh(self, case, mode, seed):
        sv = self.make()
        try:
            return self.run(sv, case, mode, seed)
        finally:
            sv.close()


def _scripted_chain(shape, hist, keep_trace, names, walk, parity, label):
    """The cases ``names[i]`` follow each other on one handle in the order ``walk``.  Case i runs scaled by 1 - 0.05 i (its own
    tolerance), from start vector i + 1, in stop mode rel / abs by the parity of i: two cases that follow each other differ in the
    script, the start, the tolerance and -- for the pairs of unlike parity, 40 of the 72 ordered pairs of nine cases -- the stop mode,
    which ``set_stop_mode`` switches between them."""
    H = _ExtHandle(shape, hist, keep_trace)
    cases = [hr.scaled(bsr.CASE[n], 1.0 - 0.05 * i) for i, n in enumerate(names)]
    modes = [("rel", "abs")[(i + parity) % 2] for i in range(len(names))]
    fresh = {}
    prev = None
    switched = 0
    try:
        for i in walk:
            got = H.run(H.sv, cases[i], modes[i], i + 1)
            if i not in fresh:
                fresh[i] = H.fresh(cases[i], modes[i], i + 1)
            want = fresh[i]
            what = (label, names[i], modes[i], "after", None if prev is None else names[prev[0]])
            _same_solve(got, want, what)
            hr.same_out(got, want, what)
            if prev is not None:
                j, a = prev
                assert not torch.equal(a["x0"], got["x0"]) and a["eps"] != got["eps"], what
                assert (a["rel_trace"][0], a["abs_trace"][0]) != (got["rel_trace"][0], got["abs_trace"][0]), what
                switched += modes[i] != modes[j]
                print(f"REUSE ext {label} A = {names[j]} ({modes[j]}): {hr.ending(a)} | B = {names[i]} ({modes[i]}): n_iter {got['n_iter']} "
                      f"stop_reason {got['stop_reason']}")
            prev = (i, got)
    finally:
        H.sv.close()
    return switched


@pytest.mark.parametrize("parity", [0, 1])
@pytest.mark.parametrize("keep_trace", [False, True], ids=["rotation", "kept"])
@pytest.mark.parametrize("hist", [torch.float32, BF16], ids=["fp32", "bf16"])
def test_scripted_solves_follow_each_other_on_one_handle(hist, keep_trace, parity, dev, monkeypatch):
    """(16, 10), every ordered pair of distinct cases of the table, 72 pairs in one walk of 73 solves on one handle.  Among them the
    A's chosen for what they leave: ``protective_break`` (prot_break = 1 and a lowest of 5e-6 that no later script reaches),
    ``lowest_not_last`` (low != cur in the rotation), ``tolerance_at_5`` (an early stop: most of the history and of both traces stay
    as the solve before filled them), ``ratio_1.31`` (history full at the threshold)."""
    for k in _KNOBS:
        monkeypatch.delenv(k, raising=False)
    names = [c.name for c in bsr.cases_for(10, "abs")]          # (the cases that are stated for both stop modes)
    assert len(names) == 9 and {"protective_break", "lowest_not_last", "tolerance_at_5", "ratio_1.31"} <= set(names)
    walk = hr.every_ordered_pair(len(names))
    switched = _scripted_chain((16, 10), hist, keep_trace, names, walk, parity, f"16x10 {'bf16' if hist == BF16 else 'fp32'}")
    assert switched == 40, switched


@functools.lru_cache(maxsize=None)
def _wide_M():
    """The smallest vector length of the recorded schedule that runs 16 floats per lane with no knob set."""
    with open(os.path.join(GOLDEN, "broyden_schedule.json")) as f:
        rows = {r["case"]: r for r in json.load(f)}
    assert rows["below_width_switch"]["M"] + 1 == rows["width_switch"]["M"]
    return rows["width_switch"]["M"]


@pytest.mark.parametrize("keep_trace", [False, True], ids=["rotation", "kept"])
@pytest.mark.parametrize("hist", [torch.float32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("size", ["409x10", "width_switch"])
def test_scripted_long_cases_follow_each_other(size, hist, keep_trace, dev, monkeypatch):
    """(409, 10) and the width switch (three sweeps, ``k_reduce_a_check``, ``a_ready`` / ``a_from`` carried from one iteration to the
    next; M = 3 << 18 is no multiple of 10: a flat handle with seq_len 1): each of ``LONG_CASES`` as A, the next of them as B; the
    modes are rel, abs, rel, rel, so the stop mode is switched in two of the three pairs."""
    for k in _KNOBS:
        monkeypatch.delenv(k, raising=False)
    if size == "409x10":
        shape = (409, 10)
    else:
        M = _wide_M()
        shape = (M // 10, 10) if M % 10 == 0 else (M, 1)
    names = list(bsr.LONG_CASES)
    switched = _scripted_chain(shape, hist, keep_trace, names, [0, 1, 2, 0], 0, f"{size} {'bf16' if hist == BF16 else 'fp32'}")
    assert switched == 2


@pytest.mark.parametrize("keep_trace", [False, True], ids=["rotation", "kept"])
@pytest.mark.parametrize("first", ["lowest_not_last", "protective_break"])
def test_a_solve_that_finds_no_lowest_iterate_returns_its_start(first, keep_trace, dev, monkeypatch):
    """B is a map that has diverged (it returns NaN): no step is ever the lowest, so what the solve returns is decided by the reset
    alone -- the reference returns x0 (``lowest_xest`` is initialised to it, nstep 0, lowest 1e8) and runs to the threshold, since no
    comparison with a NaN fires a rule.  Every other solve overwrites ``low`` at its first step, where any finite value is below 1e8:
    this is the pair that pins ``st->low = 0``.  A leaves ``low`` at a buffer other than 0 (its lowest iterate is step 3 of more)."""
    for k in _KNOBS:
        monkeypatch.delenv(k, raising=False)
    H = _ExtHandle((16, 10), torch.float32, keep_trace)

    def run(sv):
        sv.set_stop_mode("rel")
        x0 = bsr.start_vector((16, 10), device=dev, seed=7)
        return dict(sv.solve_callable(lambda x: torch.full_like(x, float("nan")), x0, 1e-3), x0=x0)
    try:
        a = H.run(H.sv, bsr.CASE[first], "rel", 1)
        assert a["nstep"] == 3 < a["n_iter"]
        got = run(H.sv)
        # judged before a fresh handle is made: on the reused handle a ``low`` that was not reset is still A's valid index
        rp = bsr.assert_replay(got, 1e-3, 45, 10, "rel", what="a map that returns NaN")
        print(f"REUSE ext nan 16x10 A = {first}: {hr.ending(a)} | B = a map that returns NaN: n_iter {got['n_iter']} stop_reason {got['stop_reason']}")
        assert (rp["stop_reason"], rp["n_iter"], rp["nstep"], rp["lowest"]) == (0, 45, 0, 1e8), rp
        assert torch.equal(got["result"], got["x0"]), "result is not the start vector"
        fresh = H.make()
        try:
            want = run(fresh)
        finally:
            fresh.close()
        hr.same_out(got, want, (first, "a map that returns NaN", "reused handle against a fresh one"))
    finally:
        H.sv.close()


# ================================================================================================ 2. natural maps, one plan each
def _build_fixture(name, tile_target):
    """The fixture's plan with two maps on it: trained weights from the stored encoder state, and seeded random weights
    (``_random``, seed 5) from h0 = 0.3 x a seeded Gaussian; for the dirichlet family also a two-layer random map."""
    eng = pkg("engine")
    dev = torch.device(DEV)
    g, mesh = load_case(name)
    mixed = CASES[name] == "mixed"
    md = mesh.to(dev)
    plan = eng.plan_for(md) if tile_target == 0 else eng.MeshPlan(md, tile_target=tile_target)
    assert bool(plan.tiled) == (tile_target != -1) and plan.N == 547
    nrm = getattr(md, "unit_normal_vector", None)
    sd_r = _random(10, mixed)
    h0r = 0.3 * torch.randn(plan.N, 10, generator=torch.Generator().manual_seed(21))
    trained = eng.FixedPointMap(plan, eng.PackedWeights(load_weights(CASES[name]), dev), torch.from_numpy(g["h0"]).to(dev), md.prb_data, nrm)
    rand = eng.FixedPointMap(plan, eng.PackedWeights(sd_r, dev), h0r.to(dev), md.prb_data, nrm)
    two = None if mixed else eng.FixedPointMap(plan, eng.PackedWeights(_random(10, False, L=2), dev), h0r.to(dev), md.prb_data, nrm)
    return dict(md=md, mesh=mesh, plan=plan, trained=trained, rand=rand, two=two, sd_r=sd_r, h0r=h0r, mixed=mixed)


@pytest.fixture(scope="module")
def fixture_maps(dev):
    """``fixture_maps(name, tile_target)`` -> ``_build_fixture``'s dictionary, built once per module and dropped after it."""
    made = {}

    def get(name, tile_target=0):
        if (name, tile_target) not in made:
            made[(name, tile_target)] = _build_fixture(name, tile_target)
        return made[(name, tile_target)]
    yield get
    for d in made.values():
        d.clear()
    made.clear()


def _recorded_step(label):
    with open(os.path.join(ROOT, "profiles", "broyden_stop_cases.json")) as f:
        return json.load(f)["solves"][label]["stagnation"]["stops_at"]


def _broyden_link(chain, name, mode, eps, solve):
    """One link of a Broyden chain: ``solve(sv)`` in ``mode`` on the reused and on a fresh handle, and the replay of its traces."""
    def run(sv):
        sv.set_stop_mode(mode)
        return solve(sv)
    out = chain.link(name, run)
    bsr.assert_replay(out, eps, 300, 10, mode, what=f"{chain.kind} {name}")
    return out


@pytest.mark.parametrize("name,tile_target", [("hex13_dirichlet_s0", 0), ("hex13_mixed_s1", 0), ("hex13_dirichlet_s0", -1)],
                         ids=["dirichlet", "mixed", "dirichlet_untiled"])
def test_natural_solves_follow_each_other_on_one_handle(name, tile_target, fixture_maps, dev):
    """One ``DeviceBroyden`` (threshold 300) per plan for a chain of forward and adjoint solves, every link beside a fresh handle.
    1 forward, trained weights, the natural-stagnation eps of ``NATURAL``; 2 forward, random weights, another h0, eps 0, stop mode
    abs (to the threshold); 3 adjoint at link 1's result (tiled VJP / gather VJP on the untiled plan, where ``plan_order`` goes to 0
    and link 6 must put it back); 4 adjoint through a linearisation rebuilt at link 2's result under link 2's weights (the mixed
    chain alternates ``"stored"`` and ``"direct"`` linearisations); 5 adjoint of a zero gradient; 6 link 1 again, link 1's bits.
    Dirichlet, tiled: a two-layer adjoint link (it allocates ``lwork``) before and after link 3."""
    eng = pkg("engine")
    F = fixture_maps(name, tile_target)
    tiled = tile_target != -1
    tr, rd = F["trained"], F["rand"]
    chain = hr.Reused(f"broyden {name}{'' if tiled else ' untiled'}", lambda: eng.DeviceBroyden(plan=F["plan"], threshold=300, keep_trace=False))
    lins = []
    try:
        label = f"forward/{name}/rel"
        eps1, thr1, reason1 = NATURAL[label][2]
        assert thr1 == 300 and reason1 == 2
        l1 = _broyden_link(chain, "1 forward trained", "rel", eps1, lambda sv: sv.solve(tr, eps1))
        if tiled:   # the recorded natural stagnation of this solver at this eps
            assert (l1["stop_reason"], l1["n_iter"]) == (reason1, _recorded_step(label)), (l1["stop_reason"], l1["n_iter"])
            assert l1["nstep"] < l1["n_iter"]
        l2 = _broyden_link(chain, "2 forward random abs", "abs", 0.0, lambda sv: sv.solve(rd, 0.0))
        assert (l2["stop_reason"], l2["n_iter"]) == (0, 300), (l2["stop_reason"], l2["n_iter"])   # history full, on every plan
        g3, g4, g2l = _seeded(l1["result"].shape, 9), _seeded(l1["result"].shape, 10, 2.0), _seeded(l1["result"].shape, 11, 0.5)
        if F["two"] is not None and tiled:
            two = F["two"]
            _broyden_link(chain, "two layers (first: allocates lwork)", "rel", 1e-4, lambda sv: sv.solve_adjoint(two, F["h0r"].to(dev), g2l, 1e-4))
        l3 = _broyden_link(chain, "3 adjoint at link 1", "rel", 1e-5, lambda sv: sv.solve_adjoint(tr, l1["result"], g3, 1e-5))
        if tiled and not F["mixed"]:   # the recorded stop of this solver at this eps
            assert NATURAL[f"adjoint/{name}/rel"][0] == (1e-5, 300, 1) and l3["stop_reason"] == 1, l3["stop_reason"]
        if F["two"] is not None and tiled:
            _broyden_link(chain, "two layers (again)", "rel", 1e-4, lambda sv: sv.solve_adjoint(two, F["h0r"].to(dev), g2l, 1e-4))
        if tiled:
            kinds = ("stored", "direct") if F["mixed"] else ("direct",)
            for n, neumann in enumerate(kinds):
                lin = rd.linearize_p(rd.to_plan(l2["result"]), neumann=neumann)
                lins.append(lin)
                assert lin.neumann_stored == (neumann == "stored" and F["mixed"])
                gr = g4 * (1.0 + n)
                _broyden_link(chain, f"4 adjoint lin {neumann} at link 2", "rel", 1e-6, lambda sv: sv.solve_adjoint(rd, l2["result"], gr, 1e-6, lin=lin))
        l5 = _broyden_link(chain, "5 adjoint zero gradient", "rel", 1e-6, lambda sv: sv.solve_adjoint(tr, l1["result"], torch.zeros_like(g3), 1e-6))
        assert (l5["stop_reason"], l5["n_iter"]) == (1, 1) and bool((l5["result"] == 0).all()), (l5["stop_reason"], l5["n_iter"])
        l6 = _broyden_link(chain, "6 link 1 again", "rel", eps1, lambda sv: sv.solve(tr, eps1))
        hr.same_out(l6, l1, (name, "link 1 again"))
        _same_solve(l6, l1, (name, "link 1 again"))
    finally:
        chain.close()
        for lin in lins:
            lin.close()


# ============================================================================================================== 3. shards
@pytest.fixture(scope="module")
def shard(dev):
    """Three dirichlet meshes ``make_hex_problem(n, seed=s)``, n = (10, 13, 26): maps with trained weights from the encoder state,
    maps with random weights from seeded starts, and trained maps from yet another start, on the same plans."""
    data, eng = pkg("data"), pkg("engine")
    dev = torch.device(DEV)
    net = pkg("model_psignn").ModelPSIGNN(dict(latent_dim=10, n_layers=1))
    net.load_state_dict(load_weights("dirichlet"))
    net = net.to(dev).eval()
    mds = [data.make_hex_problem(n, seed=s, compute_sol=False).to(dev) for s, n in enumerate((10, 13, 26))]
    with torch.no_grad():
        trained = [net.deqdss.f.bind(net.autoencoder.encoder(md.x), md) for md in mds]
    assert all(f.plan.tiled for f in trained) and max(f.plan.N for f in trained) <= 3000
    w = eng.PackedWeights(_random(10, False), dev)
    gen = torch.Generator().manual_seed(21)
    rand = [eng.FixedPointMap(f.plan, w, (0.3 * torch.randn(f.plan.N, 10, generator=gen)).to(dev), md.prb_data) for f, md in zip(trained, mds)]
    other = [eng.FixedPointMap(f.plan, f.weights, (f.h0 + 0.1 * torch.randn(f.plan.N, 10, generator=gen).to(dev)), md.prb_data)
             for f, md in zip(trained, mds)]
    total = sum(f.plan.N for f in trained) * 10
    S = dict(mds=mds, trained=trained, rand=rand, other=other, total=total)
    yield S
    S.clear()


def test_shard_solves_follow_each_other_on_the_same_handles(shard, dev):
    """``broyden_solve_batch`` with trained weights at an eps where the meshes stop at different steps, then with random weights
    (eps 0, stop mode abs), then ``broyden_solve_adjoint_batch`` at the first solve's fixed points, then a single ``solve`` of each
    handle from another start: each beside fresh handles."""
    eng = pkg("engine")
    S = shard
    tr, rd = S["trained"], S["rand"]
    chain = hr.Reused("broyden shard", lambda: [eng.DeviceBroyden(plan=f.plan, threshold=300, keep_trace=False, shard_elems=S["total"]) for f in tr])
    lins = []

    def mode(svs, m):
        for s in svs:
            s.set_stop_mode(m)
        return svs
    try:
        a = chain.link("batch trained 1e-6", lambda svs: eng.broyden_solve_batch(mode(svs, "rel"), tr, 1e-6))
        for o in a:
            bsr.assert_replay(o, 1e-6, 300, 10, "rel", what="shard trained")
        ends = [(o["stop_reason"], o["n_iter"]) for o in a]   # the meshes leave the lockstep at different steps, one of them never
        assert ends == [(1, 86), (1, 90), (0, 300)], ends
        b = chain.link("batch random abs eps 0", lambda svs: eng.broyden_solve_batch(mode(svs, "abs"), rd, 0.0))
        for o in b:
            bsr.assert_replay(o, 0.0, 300, 10, "abs", what="shard random")
        assert [(o["stop_reason"], o["n_iter"]) for o in b] == [(0, 300)] * 3, [(o["stop_reason"], o["n_iter"]) for o in b]
        lins = [f.linearize_p(f.to_plan(o["result"])) for f, o in zip(tr, a)]
        grads = [_seeded(o["result"].shape, 100 + i) for i, o in enumerate(a)]
        c = chain.link("adjoint batch", lambda svs: eng.broyden_solve_adjoint_batch(mode(svs, "rel"), lins, grads, 1e-6))
        for o in c:
            bsr.assert_replay(o, 1e-6, 300, 10, "rel", what="shard adjoint")
        assert [(o["stop_reason"], o["n_iter"]) for o in c] == [(1, 73), (1, 91), (0, 300)], [(o["stop_reason"], o["n_iter"]) for o in c]
        d = chain.link("single solves, another start", lambda svs: [s.solve(f, 1e-5) for s, f in zip(mode(svs, "rel"), S["other"])])
        for o in d:
            bsr.assert_replay(o, 1e-5, 300, 10, "rel", what="shard single")
    finally:
        chain.close()
        for lin in lins:
            lin.close()


# ================================================================================================== 4. DeviceFixedPointIter
FP_T = 30


def _fp_out(st, stop_mode):
    return dict(st, lowest=st["lowest_abs"] if stop_mode == "abs" else st["lowest"])


@pytest.mark.parametrize("shard_elems", [1 << 20, None], ids=["16_floats", "4_floats"])
def test_anderson_and_picard_follow_each_other_on_one_handle(shard_elems, fixture_maps, dev):
    """One ``DeviceFixedPointIter`` (m = 3, threshold 30) through the stepwise API: Anderson (beta 0.6, abs, an eps that stops it
    early: the updates after the stop are gated), Anderson (beta 1, rel, random weights, eps 0; its recorded points against the
    float64 recurrences), Picard (``kind`` 2 to 1), the first Anderson again."""
    eng = pkg("engine")
    F = fixture_maps("hex13_dirichlet_s0", 0)
    tr, rd = F["trained"], F["rand"]
    M = F["plan"].N * 10
    make = lambda: eng.DeviceFixedPointIter(M, dev, m=3, threshold=FP_T, shard_elems=shard_elems)
    probe = make()
    free = _stepwise_anderson(probe, tr, FP_T, 0.0, beta=0.6, stop_mode="abs")
    probe.close()
    eps_a = 1.02 * free["abs_trace"][9]      # an input of solve A, not a bound: A stops early, at or before entry 10 of 28
    chain = hr.Reused(f"fpiter {'16' if shard_elems else '4'} floats", make)
    try:
        a = chain.link("anderson beta 0.6 abs early", lambda it: _stepwise_anderson(it, tr, FP_T, eps_a, beta=0.6, stop_mode="abs"))
        assert a["stop_reason"] == 1 and a["n_iter"] <= 10 < FP_T - 2, (a["stop_reason"], a["n_iter"])
        rec = rc.Recorder(rd.fp)
        b = chain.link("anderson beta 1 rel random eps 0", lambda it: _stepwise_anderson(it, rd, FP_T, 0.0, beta=1.0, stop_mode="rel", F=rec))
        # (the recorder holds the reused handle's run first, the fresh handle's after it)
        n = rc.check_anderson(rec.P[:FP_T], rec.R[:FP_T], _fp_out(b, "rel"), 3, 1e-4, 1.0, FP_T, 0.0, "rel", where="reused handle")
        assert n == FP_T - 2 == b["n_iter"]
        p = chain.link("picard", lambda it: _stepwise_picard(it, tr, FP_T, 0.0))
        assert p["n_iter"] == FP_T + 1, p["n_iter"]
        a2 = chain.link("anderson beta 0.6 abs early, again", lambda it: _stepwise_anderson(it, tr, FP_T, eps_a, beta=0.6, stop_mode="abs"))
        hr.same_out(a2, a, "the first Anderson solve again")
    finally:
        chain.close()


def test_lockstep_anderson_and_picard_follow_each_other(shard, dev):
    """The same alternation through ``anderson_solve_batch`` / ``picard_solve_batch`` on the handles of the three-mesh shard."""
    eng = pkg("engine")
    S = shard
    tr, rd = S["trained"], S["rand"]
    make = lambda: [eng.DeviceFixedPointIter(f.plan.N * 10, dev, m=3, threshold=FP_T, shard_elems=S["total"]) for f in tr]
    probe = make()
    free = eng.anderson_solve_batch(probe, tr, 0.0, beta=0.6, stop_mode="abs")
    hr.Reused.close_one(probe)
    eps_a = 1.02 * free[0]["abs_trace"][9]
    chain = hr.Reused("fpiter shard", make)
    try:
        a = chain.link("anderson beta 0.6 abs early", lambda its: eng.anderson_solve_batch(its, tr, eps_a, beta=0.6, stop_mode="abs"))
        # mesh 0 stops where eps_a was taken, mesh 1 later, mesh 2 runs all 28 passes while the others' updates are gated
        assert [(o["stop_reason"], o["n_iter"]) for o in a] == [(1, 10), (1, 17), (0, FP_T - 2)], [(o["stop_reason"], o["n_iter"]) for o in a]
        b = chain.link("anderson beta 1 rel random eps 0", lambda its: eng.anderson_solve_batch(its, rd, 0.0, beta=1.0, stop_mode="rel"))
        assert all(o["n_iter"] == FP_T - 2 for o in b)
        p = chain.link("picard", lambda its: eng.picard_solve_batch(its, tr, 0.0))
        assert all(o["n_iter"] == FP_T + 1 for o in p)
        a2 = chain.link("anderson beta 0.6 abs early, again", lambda its: eng.anderson_solve_batch(its, tr, eps_a, beta=0.6, stop_mode="abs"))
        for i, (x, y) in enumerate(zip(a2, a)):
            hr.same_out(x, y, ("the first lockstep Anderson solve again", i))
    finally:
        chain.close()


# ============================================================================================================ 5. DeviceGmres
GM = 12
# B of the single-handle pairs: the random-weight system falls by about a decade per product (1e-7 after 14), so its budget ends it in
# the middle of the first cycle, four Arnoldi steps in, well above the fp32 floor where a comparison with float64 says something
GM_EPS_B, GM_BUDGET_B = 1e-12, 5


@pytest.fixture(scope="module")
def gmres_problem(fixture_maps, dev):
    """A: the dirichlet fixture's trained map linearised at its fixed point (eps 1e-5 / 300) with a seeded gradient.  B: the random
    map linearised at its start h0r, twice the gradient of another seed."""
    eng = pkg("engine")
    F = fixture_maps("hex13_dirichlet_s0", 0)
    tr, rd = F["trained"], F["rand"]
    sv = eng.DeviceBroyden(plan=F["plan"], threshold=300, keep_trace=False)
    H = sv.solve(tr, 1e-5)["result"]
    sv.close()
    HB = F["h0r"].to(DEV)
    P = dict(F=F, H=H, g=_seeded(H.shape, 9), lin=tr.linearize_p(tr.to_plan(H)), HB=HB, gB=_seeded(H.shape, 10, 2.0),
             linB=rd.linearize_p(rd.to_plan(HB)))
    yield P
    P["lin"].close()
    P["linB"].close()
    P.clear()


def _gmres_stepwise_three(sv, P):
    """The stepwise API left after three Arnoldi steps: begin, three products through the stored linearisation, one solution."""
    tr = P["F"]["trained"]
    shape = tuple(P["H"].shape)
    sv.begin(tr.to_plan(P["g"]))
    for j in range(3):
        P["lin"].jvp_p(sv.row(j, shape), out=sv.row(j + 1, shape))
        sv.step(j, 1.0, 1e-6)
    z = torch.empty_like(P["H"])
    kk, beta, resid = sv.solution(None, 1.0, z, info=True)
    assert kk == 3 and resid < beta, (kk, beta, resid)


@pytest.mark.parametrize("first", ["budget_mid_cycle", "tolerance", "zero_gradient", "stepwise_three"])
def test_gmres_adjoint_after_another_solve(first, gmres_problem, dev):
    """``DeviceGmres`` (m = 12): after A -- a budget that runs out six steps into the second restart cycle, a tolerance stop, the zero
    gradient (|b| = 0), the stepwise API left after three steps -- B is ``solve_adjoint`` with another gradient, a linearisation at
    another state under other weights, another eps and budget (5: four Arnoldi steps, then the budget).  B equals B on a fresh handle,
    and after the first A it is also held against the float64 restatement."""
    eng = pkg("engine")
    P = gmres_problem
    tr, rd = P["F"]["trained"], P["F"]["rand"]
    chain = hr.Reused(f"gmres after {first}", lambda: eng.DeviceGmres(P["F"]["plan"].N * 10, dev, GM))
    try:
        if first == "budget_mid_cycle":
            a = chain.link("A budget 20", lambda sv: sv.solve_adjoint(tr, P["H"], P["g"], 1e-8, 20, lin=P["lin"]), compare=False)
            assert (a["stop"], a["nstep"], a["n_cycles"]) == ("budget", 20, 3), (a["stop"], a["nstep"], a["n_cycles"])
        elif first == "tolerance":
            a = chain.link("A eps 1e-4", lambda sv: sv.solve_adjoint(tr, P["H"], P["g"], 1e-4, 500, lin=P["lin"]), compare=False)
            assert a["stop"] == "tolerance" and a["lowest"] < 1e-4, (a["stop"], a["lowest"])
        elif first == "zero_gradient":
            a = chain.link("A zero gradient", lambda sv: sv.solve_adjoint(tr, P["H"], torch.zeros_like(P["g"]), 1e-8, 500, lin=P["lin"]), compare=False)
            assert (a["stop"], a["nstep"], a["n_cycles"]) == ("tolerance", 0, 1) and bool((a["result"] == 0).all())
        else:
            _gmres_stepwise_three(chain.h, P)
            chain.follow("A stepwise, three steps", None)
        b = chain.link("B other gradient, state, weights", lambda sv: sv.solve_adjoint(rd, P["HB"], P["gB"], GM_EPS_B, GM_BUDGET_B, lin=P["linB"]))
        assert (b["stop"], b["nstep"], b["n_cycles"]) == ("budget", GM_BUDGET_B, 2), (b["stop"], b["nstep"], b["n_cycles"])
        if first == "budget_mid_cycle":
            F = P["F"]
            fm64 = eng.FixedPointMap64(F["plan"], eng.PackedWeights64(F["sd_r"], dev), F["h0r"].to(dev), F["md"].prb_data, F["md"].edge_attr)
            try:
                t32 = ref.gmres_adjoint(lambda v: rd.from_plan(P["linB"].vjp_p(rd.to_plan(v))), P["gB"], GM_EPS_B, GM_BUDGET_B, m=GM, device=dev)
                t64 = ref.gmres_adjoint(lambda v: fm64.vjp(P["HB"], v), P["gB"].double(), GM_EPS_B, GM_BUDGET_B, m=GM, device=dev)
            finally:
                fm64.close()
            hr.gmres_against_restatement("B on the reused handle", b, t64, t32)
    finally:
        chain.close()


def test_gmres_shard_and_single_solves_follow_each_other(shard, dev):
    """Handles made with ``shard_elems`` for the three-mesh shard: single solves, then ``gmres_solve_adjoint_batch`` with other
    gradients, eps and budget, then single solves again -- the lockstep solve after single ones and the reverse."""
    eng = pkg("engine")
    S = shard
    tr = S["trained"]
    svs = [eng.DeviceBroyden(plan=f.plan, threshold=300, keep_trace=False, shard_elems=S["total"]) for f in tr]
    H = [o["result"] for o in eng.broyden_solve_batch(svs, tr, 1e-5)]
    hr.Reused.close_one(svs)
    lins = [f.linearize_p(f.to_plan(h)) for f, h in zip(tr, H)]
    g1 = [_seeded(h.shape, 100 + i) for i, h in enumerate(H)]
    g2 = [_seeded(h.shape, 200 + i, 3.0) for i, h in enumerate(H)]
    g3 = [_seeded(h.shape, 300 + i, 0.5) for i, h in enumerate(H)]
    chain = hr.Reused("gmres shard", lambda: [eng.DeviceGmres(f.plan.N * 10, dev, GM, shard_elems=S["total"]) for f in tr])
    try:
        a = chain.link("single eps 1e-4", lambda svs: [s.solve_adjoint(f, h, g, 1e-4, 200, lin=l) for s, f, h, g, l in zip(svs, tr, H, g1, lins)])
        assert [(o["stop"], o["nstep"]) for o in a] == [("tolerance", 35), ("tolerance", 39), ("stagnation", 52)], [(o["stop"], o["nstep"]) for o in a]
        assert eng.gmres_adjoint_batchable(chain.h, lins)
        b = chain.link("batch budget 20", lambda svs: eng.gmres_solve_adjoint_batch(svs, lins, g2, 1e-8, 20))
        # (mesh 2's second cycle does not halve its residual: its head of cycle 2, at the budget, reports the stagnation first)
        assert [(o["stop"], o["nstep"]) for o in b] == [("budget", 20), ("budget", 20), ("stagnation", 20)], [(o["stop"], o["nstep"]) for o in b]
        chain.link("single eps 1e-5", lambda svs: [s.solve_adjoint(f, h, g, 1e-5, 200, lin=l) for s, f, h, g, l in zip(svs, tr, H, g3, lins)])
    finally:
        chain.close()
        for lin in lins:
            lin.close()


# ================================================================================================================ 6. float64
def _p64(dev):
    from test_gpu_f64 import fixture_problem
    return fixture_problem("hex13_dirichlet_s0", dev)


def test_float64_broyden_solves_follow_each_other(dev):
    """``DeviceBroyden64``: ``solve`` (the tolerance stop of ``NATURAL64``), ``solve_adjoint`` at its result, ``solve`` from another
    x0 at another eps; each beside a fresh handle on the same ``FixedPointMap64`` and against the replay of its traces."""
    eng = pkg("engine")
    p = _p64(dev)
    eps1, thr, reason = NATURAL64["forward64/hex13_dirichlet_s0/rel"][0]
    chain = hr.Reused("broyden64", lambda: eng.DeviceBroyden64(p.fmap, thr))
    try:
        h0 = p.h0.to(dev)
        a = chain.link("solve", lambda sv: sv.solve(h0, eps1))
        assert bsr.assert_replay(a, eps1, thr, 10, "rel", what="broyden64 solve")["stop_reason"] == reason
        g = _seeded(h0.shape, 9, dtype=torch.float64)
        b = chain.link("solve_adjoint", lambda sv: sv.solve_adjoint(a["result"], g, 1e-9))
        bsr.assert_replay(b, 1e-9, thr, 10, "rel", what="broyden64 adjoint")
        x0 = h0 + _seeded(h0.shape, 12, 0.05, dtype=torch.float64)
        c = chain.link("solve from another x0", lambda sv: sv.solve(x0, 1e-8))
        bsr.assert_replay(c, 1e-8, thr, 10, "rel", what="broyden64 other x0")
    finally:
        chain.close()


def test_float64_gmres_solves_follow_each_other(dev):
    """``DeviceGmres64`` (m = 12): a budget that runs out inside the second cycle, then another gradient to a tolerance."""
    eng = pkg("engine")
    p = _p64(dev)
    h0 = p.h0.to(dev)
    chain = hr.Reused("gmres64", lambda: eng.DeviceGmres64(p.fmap, GM))
    try:
        a = chain.link("budget 20", lambda sv: sv.solve_adjoint(h0, _seeded(h0.shape, 9, dtype=torch.float64), 1e-13, 20))
        assert (a["stop"], a["nstep"]) == ("budget", 20), (a["stop"], a["nstep"])
        b = chain.link("another gradient", lambda sv: sv.solve_adjoint(h0, _seeded(h0.shape, 10, 2.0, dtype=torch.float64), 1e-6, 300))
        assert b["stop"] == "tolerance", b["stop"]
    finally:
        chain.close()


def test_poisson_cg_solves_follow_each_other(shard, dev):
    """``PoissonCG``: ``solve(y1)``, ``solve(y2, x0=...)`` at another tolerance, ``solve(y1)`` again with the first solve's bits."""
    eng = pkg("engine")
    md = shard["mds"][1]
    plan = eng.plan_for(md)
    chain = hr.Reused("poisson cg", lambda: eng.PoissonCG(plan, md.a_ij))
    try:
        y1 = md.y
        y2 = 1.7 * md.y.double() + _seeded(md.y.shape, 5, 0.3, dtype=torch.float64)
        x0 = _seeded(md.y.shape, 6, dtype=torch.float64)
        a = chain.link("solve y1", lambda cg: cg.solve(y1))
        assert a["converged"]
        b = chain.link("solve y2 from x0", lambda cg: cg.solve(y2, x0=x0, tol=1e-6))
        assert b["converged"]
        c = chain.link("solve y1 again", lambda cg: cg.solve(y1))
        hr.same_out(c, a, "the first solve again")
    finally:
        chain.close()
