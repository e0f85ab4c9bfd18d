"""GPU: the float64 adjoint solves on the device (``psignn_gmres64_*``, ``psignn_broyden64_solve_adjoint``; ``engine.DeviceGmres64``,
``DeviceBroyden64.solve_adjoint``, ``adjoint64``) against the float64 CPU oracle: the GMRES restatement
``adjoint_gmres_ref.gmres_adjoint`` on ``AdjointProblem.vjp64``, ``orc.broyden`` under a float64 default dtype, and ``truth()``.

Problems: ``adjoint_gmres_ref.AdjointProblem`` (H* from the oracle's fp32 Broyden, ``grad`` seed 0); device maps: ``test_gpu_f64.Problem``.

Where the gates come from (the rule of tests/test_gpu_f64.py).  scripts/calib_f64_adjoint.py multiplies every product of the float64
oracle by 1 + s * 2^-52, s uniform in [-4, 4] per element -- the freedom a correct float64 statement with another summation order
has -- and runs both CPU solves again, three seeds (eps 1e-11; GMRES m 50, budget 2000; Broyden threshold 800):

====================  ===========================  ==========  =============  ===============  ===========================  ====================
fixture               GMRES products/cycles/stop   result      trace entries  lowest vs true   Broyden steps (perturbed)    Broyden result to
                      (none moved, n_reorth too)   moved       moved (abs)    residual (rel)   entries 0-9 moved; first >   truth() (base; pert.)
                                                                                               1e-10
====================  ===========================  ==========  =============  ===============  ===========================  ====================
hex13_dirichlet_s0    98 / 3 / tolerance (95)      <= 2.1e-15  <= 2.6e-15     <= 3.9e-6        157 (145 - 159) 1.7e-14; 20  1.1e-10; <= 1.6e-10
hex26_dirichlet_s0    225 / 6 / tolerance (215)    <= 9.8e-15  <= 1.0e-14     <= 3.2e-6        506 (459 - 475) 1.8e-14; 19  5.7e-10; <= 5.1e-10
hex13_mixed_s1        153 / 4 / tolerance (146)    <= 6.1e-15  <= 9.6e-15     <= 4.1e-6        180 (179 - 200) 1.2e-13; 24  1.1e-10; <= 3.7e-10
hex13, two layers     11 / 2 / tolerance (9)       <= 5.0e-17  <= 1.4e-16     <= 6.4e-7        11 (11)                      3.0e-12 (GMRES 3.6e-12)
====================  ===========================  ==========  =============  ===============  ===========================  ====================

(The counts of a fixture depend on H*, which comes from a chaotic fp32 Broyden solve on the CPU: another host may see, say, 223
products on hex26.  The tests compare the device with the restatement run on the same H* in the same process.  The moved trace
entries are absolute: the large ones, |grad| ~ 1e2, move by 1e-14, the ones at 5e-12 by 3e-17, which is up to 7e-6 relative.)

* GMRES (test 1): products, cycles and stop reason equal the restatement's; the result within 2.5e-12 relative L2 of it (250 x the
  worst perturbed distance, 9.8e-15); trace entries |a - b| <= 1e-12 b + 1e-14 (the absolute term is the worst movement seen, the
  relative one 250 x 2^-52 rounded up, for the large entries); ``lowest`` = the oracle's float64 residual of the device result at
  rtol 1e-4 (an entry at 5e-12 is the difference of vectors with entries O(1), so it moves by 4e-6 relative; 25 x that).
  ``n_reorth`` is printed.
* stop reasons (test 2): (m, budget) pairs for which the restatement, run in the test, ends on the reason named; the device must
  end the same way with the same counts.
* Broyden (test 4): entries 0-9 of both traces at rtol 1e-9 (moved by <= 1.2e-13; the first to move by more than 1e-10 is number
  19); ``lowest`` < 1e-11 and no protective break; the result within 1e-8 of ``truth()`` (10 x the worst distance of the oracle's
  own solves over hosts, 1.0e-9; 5.7e-10 here); ``lowest`` = the oracle's residual of the result at rtol 1e-4, the gate of the
  GMRES ``lowest``, which is the same quantity -- a norm of 1e-11 of the difference of two vectors with entries O(1): under the
  perturbation the oracle's own Broyden ``lowest`` is 6e-8 - 2.3e-6 relative from the unperturbed residual of its result (so a
  gate of 1e-6 is inside the spread; the device measured 1.4e-6 on hex13_mixed_s1).  Step counts are printed: Broyden trajectories
  are chaotic.
* two layers (test 5): traces move by 1e-7 relative as they reach 1e-12 and are not compared; both results within 3.6e-11 of
  ``truth()``, 10 x the CPU solves' own 3.0e-12 / 3.6e-12.
* 10 981 nodes (test 6): no claim about convergence; what the solvers report must be what their results have.

On the MI355X, one run: the GMRES results are 2.5e-15 / 1.1e-14 / 1.2e-14 from the restatement's, trace entries within 4.3e-13
absolute (on |grad| = 145) and 3.0e-6 relative (on 5e-12); Broyden traces 0-9 within 1.1e-13, results 1.3e-10 / 1.3e-9 / 4.3e-10
from ``truth()`` after 151 / 495 / 199 steps.
"""
import os

import numpy as np
import pytest
import torch

import adjoint_gmres_ref as ref
from conftest import GOLDEN, load_weights, pkg, rel_l2
from oracle import psignn_oracle as orc
from test_gpu_f64 import Problem, fixture_problem, float64_default

pytestmark = pytest.mark.gpu

EPS = 1e-11
_cache = {}


class Pair:
    """One adjoint problem on the CPU oracle and the device map of the same mesh and weights."""

    def __init__(self, name, dev, sd=None):
        self.ap = ref.AdjointProblem(name, sd=sd)
        self.dp = Problem(self.ap.mesh, self.ap.sd, dev, h0=self.ap.h0.double())
        self.dev = dev
        self.hs, self.grad = self.ap.h_star.to(dev), self.ap.grad.to(dev)   # float32: widened exactly by the engine
        self._gm, self._by, self._ref = {}, {}, {}

    def gmres(self, m):
        if m not in self._gm:
            self._gm[m] = self.dp.eng.DeviceGmres64(self.dp.fmap, m)
        return self._gm[m]

    def broyden(self, threshold):
        if threshold not in self._by:
            self._by[threshold] = self.dp.eng.DeviceBroyden64(self.dp.fmap, threshold)
        return self._by[threshold]

    def gmres_cpu(self, m, max_products):
        key = (m, max_products)
        if key not in self._ref:
            self._ref[key] = ref.gmres_adjoint(self.ap.vjp64, self.ap.grad.double(), EPS, max_products, m=m)
        return self._ref[key]

    def broyden_cpu(self, threshold):
        g64 = self.ap.grad.double()
        with float64_default(), torch.no_grad():
            return orc.broyden(lambda y: self.ap.vjp64(y) + g64, torch.zeros_like(g64), threshold=threshold, eps=EPS)

    def residual_cpu(self, y):
        """rel of both solvers at y on the float64 oracle: |f(y) - y| / (|f(y)| + 1e-9), f(y) = J^T y + grad."""
        y = y.detach().cpu().double()
        f = self.ap.vjp64(y) + self.ap.grad.double()
        return float((f - y).norm()) / (float(f.norm()) + 1e-9)


def pair(name, dev):
    if name not in _cache:
        _cache[name] = Pair(name, dev)
    return _cache[name]


def two_layer_pair(dev):
    if "two layers" not in _cache:
        _cache["two layers"] = Pair("hex13_dirichlet_s0", dev, sd=ref.stacked_dirichlet(2))
    return _cache["two layers"]


def _same_run(a, b, what):
    assert torch.equal(a["result"], b["result"]), what
    assert a["rel_trace"] == b["rel_trace"] and a["abs_trace"] == b["abs_trace"], what
    for k in ("nstep", "lowest", "n_iter", "n_cycles", "stop", "n_reorth", "stop_reason"):
        assert a.get(k) == b.get(k), (what, k)


# ----------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("name", ref.FIXTURES)
def test_gmres_against_the_restatement(name, dev):
    p = pair(name, dev)
    want = p.gmres_cpu(50, 2000)
    got = p.gmres(50).solve_adjoint(p.hs, p.grad, EPS, 2000)
    dist = rel_l2(got["result"], want["result"])
    res = p.residual_cpu(got["result"])
    print(f"F64A {name} GMRES: device products {got['nstep']} cycles {got['n_cycles']} stop {got['stop']} n_reorth {got['n_reorth']} "
          f"lowest {got['lowest']:.6e}; restatement {want['nstep']} / {want['n_cycles']} / {want['stop']} / {want['n_reorth']} "
          f"lowest {want['lowest']:.6e}; distance {dist:.2e}; oracle's residual of the device result {res:.6e}; "
          f"distance to truth {p.ap.error(got['result']):.2e}")
    assert want["stop"] == "tolerance"
    assert got["result"].dtype == torch.float64 and got["result"].shape == p.ap.grad.shape
    assert (got["nstep"], got["n_cycles"], got["stop"]) == (want["nstep"], want["n_cycles"], want["stop"])
    assert dist <= 2.5e-12
    for tr in ("rel_trace", "abs_trace"):
        a, b = np.array(got[tr]), np.array(want[tr])
        assert a.shape == b.shape == (want["n_cycles"],)
        print(f"F64A {name} {tr}: max |a - b| {float(np.max(np.abs(a - b))):.2e}, max rel {float(np.max(np.abs(a - b) / b)):.2e}")
        assert np.all(np.abs(a - b) <= 1e-12 * b + 1e-14), (tr, a, b)
    np.testing.assert_allclose(got["lowest"], res, rtol=1e-4)
    assert got["lowest"] == min(got["rel_trace"])


# ----------------------------------------------------------------------------------------------------------------- 2
# (m, budget).  stagnation: two steps of the second cycle cannot halve what eight steps left; budget: the second cycle's residual is
# product 51 and one product is kept back, so no step is left, whatever the residual (it is ~1e-5, far from eps)
STOPS = {"stagnation": (8, 12), "budget": (50, 52), "tolerance": (50, 2000)}


@pytest.mark.parametrize("stop", sorted(STOPS))
@pytest.mark.parametrize("name", ref.FIXTURES)
def test_gmres_stops_as_the_restatement_does(name, stop, dev):
    p = pair(name, dev)
    m, budget = STOPS[stop]
    want = p.gmres_cpu(m, budget)
    assert want["stop"] == stop, (want["stop"], want["nstep"], want["n_cycles"])   # the case is what it is meant to be
    got = p.gmres(m).solve_adjoint(p.hs, p.grad, EPS, budget)
    print(f"F64A {name} m {m} budget {budget}: device {got['nstep']} / {got['n_cycles']} / {got['stop']} / n_reorth {got['n_reorth']}, "
          f"restatement {want['nstep']} / {want['n_cycles']} / {want['stop']} / n_reorth {want['n_reorth']}")
    assert (got["nstep"], got["n_cycles"], got["stop"]) == (want["nstep"], want["n_cycles"], want["stop"])
    assert got["nstep"] <= budget and len(got["rel_trace"]) == got["n_cycles"]
    assert rel_l2(got["result"], want["result"]) <= 2.5e-12


# ----------------------------------------------------------------------------------------------------------------- 3
def test_zero_gradient(dev):
    p = pair("hex13_dirichlet_s0", dev)
    zero = torch.zeros_like(p.grad)
    got = p.gmres(50).solve_adjoint(p.hs, zero, EPS, 2000)
    assert got["nstep"] == 0 and got["n_cycles"] == 1 and got["stop"] == "tolerance" and got["lowest"] == 0.0
    assert got["result"].dtype == torch.float64 and not bool(got["result"].any())


# ----------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("name", ref.FIXTURES)
def test_broyden_against_the_oracle(name, dev):
    p = pair(name, dev)
    got = p.broyden(800).solve_adjoint(p.hs, p.grad, EPS)
    want = p.broyden_cpu(10)
    assert got["n_iter"] >= 10
    for tr in ("rel_trace", "abs_trace"):
        a, b = np.array(got[tr][:10]), np.array(want[tr][:10])
        print(f"F64A {name} Broyden {tr}[:10] max rel diff {float(np.max(np.abs(a - b) / b)):.2e}")
        np.testing.assert_allclose(a, b, rtol=1e-9, atol=0)
    err, res = p.ap.error(got["result"]), p.residual_cpu(got["result"])
    print(f"F64A {name} Broyden: n_iter {got['n_iter']} nstep {got['nstep']} lowest {got['lowest']:.3e} stop {got['stop_reason']}; "
          f"distance to truth {err:.2e}; oracle's residual of the result {res:.3e}")
    assert got["result"].dtype == torch.float64
    assert got["lowest"] < 1e-11 and not got["prot_break"]
    assert err <= 1e-8
    np.testing.assert_allclose(got["lowest"], res, rtol=1e-4)


# ----------------------------------------------------------------------------------------------------------------- 5
def test_two_layers(dev):
    p = two_layer_pair(dev)
    assert p.dp.w.n_layers == 2
    g = p.gmres(50).solve_adjoint(p.hs, p.grad, EPS, 2000)
    b = p.broyden(800).solve_adjoint(p.hs, p.grad, EPS)
    eg, eb = p.ap.error(g["result"]), p.ap.error(b["result"])
    print(f"F64A two layers: GMRES products {g['nstep']} cycles {g['n_cycles']} stop {g['stop']} lowest {g['lowest']:.3e} to truth {eg:.2e}; "
          f"Broyden n_iter {b['n_iter']} lowest {b['lowest']:.3e} to truth {eb:.2e}")
    assert g["stop"] == "tolerance" and b["lowest"] < 1e-11 and not b["prot_break"]
    assert eg <= 3.6e-11 and eb <= 3.6e-11


# ----------------------------------------------------------------------------------------------------------------- 6
@pytest.mark.parametrize("mixed", [False, True])
def test_many_blocks_ragged_tail(mixed, dev):
    """10 981 nodes at the encoder state: 109 810 elements are 215 blocks of 512 and 108 chunks of 1 024, both with a ragged tail.
    No claim about convergence; what the solvers report must be what their results have."""
    eng = pkg("engine")
    mesh = pkg("data").make_hex_problem(60, seed=3, mixed=mixed, compute_sol=False)
    assert mesh.num_nodes == 10981
    p = Problem(mesh, load_weights("mixed" if mixed else "dirichlet"), dev)
    H = p.h0.to(dev)
    grad = torch.randn(H.shape, generator=torch.Generator().manual_seed(0)).to(dev)

    def residual(y):
        f = p.fmap.vjp(H, y, grad)
        return float((f - y).norm()) / (float(f.norm()) + 1e-9)

    fam = "mixed" if mixed else "dirichlet"
    gm = eng.DeviceGmres64(p.fmap, 30)
    g = gm.solve_adjoint(H, grad, EPS, 120)
    rg = residual(g["result"])
    print(f"F64A hex60 {fam} GMRES: products {g['nstep']} cycles {g['n_cycles']} stop {g['stop']} n_reorth {g['n_reorth']} "
          f"lowest {g['lowest']:.6e} recomputed {rg:.6e}")
    np.testing.assert_allclose(g["lowest"], rg, rtol=1e-6)
    assert g["nstep"] <= 120 and g["lowest"] == min(g["rel_trace"]) and len(g["rel_trace"]) == g["n_cycles"]
    assert gm.nbytes >= 31 * H.numel() * 8
    gm.close()
    by = eng.DeviceBroyden64(p.fmap, 60)
    b = by.solve_adjoint(H, grad, EPS)
    rb = residual(b["result"])
    print(f"F64A hex60 {fam} Broyden: n_iter {b['n_iter']} nstep {b['nstep']} lowest {b['lowest']:.6e} recomputed {rb:.6e} "
          f"stop {b['stop_reason']}")
    np.testing.assert_allclose(b["lowest"], rb, rtol=1e-6)
    trace = b["rel_trace"]
    assert 1 <= b["nstep"] <= b["n_iter"] <= 60 and len(trace) == 61
    assert trace[b["nstep"] - 1] == b["lowest"] == min(trace)
    by.close()


# ----------------------------------------------------------------------------------------------------------------- 7
def test_same_bits(dev):
    p = pair("hex13_dirichlet_s0", dev)
    gm, by = p.gmres(50), p.broyden(800)
    first = gm.solve_adjoint(p.hs, p.grad, EPS, 2000)
    for pe in (1, 64):
        _same_run(gm.solve_adjoint(p.hs, p.grad, EPS, 2000, poll_every=pe), first, f"GMRES poll_every {pe}")
    first = by.solve_adjoint(p.hs, p.grad, EPS)
    for pe in (1, 64):
        _same_run(by.solve_adjoint(p.hs, p.grad, EPS, poll_every=pe), first, f"Broyden poll_every {pe}")
    # float64 inputs are the float32 ones widened
    _same_run(gm.solve_adjoint(p.hs.double(), p.grad.double(), EPS, 2000), gm.solve_adjoint(p.hs, p.grad, EPS, 2000), "float64 inputs")


def test_forward_solve_keeps_the_parent_bits(dev):
    """``psignn_broyden64_solve`` on hex13 from h0 (eps 1e-11, threshold 1000), now one loop over an operator shared with the
    adjoint solve: result, traces and counts bit-equal to the build before that (tests/golden/broyden64_hex13_parent.npz, recorded
    on the MI355X from that build)."""
    rec = np.load(os.path.join(GOLDEN, "broyden64_hex13_parent.npz"))
    p = fixture_problem("hex13_dirichlet_s0", dev)
    out = p.solver(1000).solve(p.h0.to(dev), 1e-11)
    n = int(rec["n_iter"])
    assert (out["n_iter"], out["nstep"], out["stop_reason"]) == (n, int(rec["nstep"]), int(rec["stop_reason"]))
    assert np.array_equal(np.array(out["rel_trace"][:n]), rec["rel_trace"])
    assert np.array_equal(np.array(out["abs_trace"][:n]), rec["abs_trace"])
    assert np.array_equal(out["result"].cpu().numpy(), rec["result"])
    assert out["lowest"] == float(rec["lowest"])


# ----------------------------------------------------------------------------------------------------------------- 8
def test_adjoint64_and_refusals_on_open_handles(dev):
    nat, eng = pkg("_native"), pkg("engine")
    p = pair("hex13_dirichlet_s0", dev)
    md = p.ap.mesh.to(dev)
    want = p.gmres(50).solve_adjoint(p.hs, p.grad, EPS, 2000)
    got = eng.adjoint64(md, p.ap.sd, p.hs, p.grad)
    # the convenience encodes h0 in float64 itself; J does not depend on h0 (Dirichlet rows are constants), so the bits agree
    assert torch.equal(got["result"], want["result"]) and got["nstep"] == want["nstep"]
    by = eng.adjoint64(md, p.ap.sd, p.hs, p.grad, solver="broyden", threshold=300)
    assert by["lowest"] < 1e-11 and p.ap.error(by["result"]) <= 1e-8
    # a workspace that is too small is an error code naming the bytes; a restart length out of range too
    fm, lib = p.dp.fmap, nat.lib()
    need = lib.psignn_f64_deriv_workspace_doubles(fm.handle, 1, 1)
    work = torch.zeros(need, dtype=torch.float64, device=dev)
    hs, gr, out = p.hs.double(), p.grad.double(), torch.zeros_like(p.grad, dtype=torch.float64)
    info = nat.GmresAdjointInfo()
    args = lambda n: (p.gmres(50).handle, nat.ptr(fm.wflat), 1, nat.ptr(hs), nat.ptr(fm.h0), nat.ptr(fm.prb), None, nat.ptr(gr),
                      EPS, 20, 8, nat.ptr(work), n, nat.ptr(out), info, None, None, None)
    assert lib.psignn_gmres64_solve_adjoint(*args(need - 1)) < 0
    assert f"{need * 8} bytes" in lib.psignn_last_error().decode()
    assert lib.psignn_gmres64_solve_adjoint(*args(need)) == 0 and info.products <= 20
    import ctypes
    h = ctypes.c_void_p()
    assert lib.psignn_gmres64_create(ctypes.byref(h), fm.handle, 0) < 0 and not h.value
    with pytest.raises(nat.NativeError, match="restart length out of range"):
        eng.DeviceGmres64(fm, 4097)   # refused before any allocation is tried
