"""Forward inference at latent widths 8 and 16 (libpsignn_hip_d8.so / _d16.so) on the GPU against the CPU oracle in float64.

Weights: seeded random blocks, the recipe of tests/test_gpu_multilayer.py::_random -- ``torch.manual_seed(5)``, the family's
``ModelPSIGNN(dict(latent_dim=d, n_layers=1))``, ``normal_(std=0.1)`` on every 1-D parameter.  With these the oracle alone
(float32, fw_tol 1e-7, fw_thres 600) converges in 13 / 32 (hex13_dirichlet_s0, d = 8 / 16), 12 / 14 (hex13_mixed_s1) and
13 / 40 (hex26_dirichlet_s0) Broyden steps without a protective break, its float32 fixed point within 3.3e-7 of the float64
one and its float32 single f within 8e-8: the gates below are the project's existing ones (single f 2e-6, encoder 1e-6,
converged node states and decoded u 1e-5) and need no widening.  Nothing here provokes an error on the device: every refusal
is decided on the host."""
import numpy as np
import pytest
import torch

import limit_graphs as lg
from conftest import load_case, load_weights, pkg, rel_l2
from oracle import psignn_oracle as orc

pytestmark = pytest.mark.gpu

WIDTHS = (8, 16)
FIXTURES = ("hex13_dirichlet_s0", "hex13_mixed_s1", "hex26_dirichlet_s0")
ORACLE_STEPS = {("hex13_dirichlet_s0", 8): 13, ("hex13_dirichlet_s0", 16): 32, ("hex13_mixed_s1", 8): 12,
                ("hex13_mixed_s1", 16): 14, ("hex26_dirichlet_s0", 8): 13, ("hex26_dirichlet_s0", 16): 40}


def _mod(mixed):
    return pkg("mixed") if mixed else pkg("model_psignn")


def _random(d, mixed, L=1, seed=5):
    torch.manual_seed(seed)
    net = _mod(mixed).ModelPSIGNN(dict(latent_dim=d, n_layers=L))
    for p in net.parameters():
        if p.dim() == 1:
            torch.nn.init.normal_(p, std=0.1)
    return {k: v.detach().clone() for k, v in net.state_dict().items()}


def _mesh64(mesh):
    m = mesh.clone()
    for k, v in list(vars(mesh).items()):
        if torch.is_tensor(v) and v.is_floating_point():
            setattr(m, k, v.double())
    return m


def _sd64(sd):
    return {k: v.double() for k, v in sd.items()}


def _dirichlet_rows(mesh, mixed):
    t = mesh.tags[:, 1] if mixed else mesh.tags.reshape(mesh.num_nodes, -1)[:, 0]
    return torch.where(t == 1)[0]


def _setup(mesh, sd, d, mixed, dev, tile_target=0, seed=11):
    """(fmap, h0, h): h random with h0's Dirichlet rows; h0 = the encoder of the mesh's input (_setup of test_gpu_multilayer)."""
    eng = pkg("engine")
    md = mesh.to(dev)
    with torch.no_grad():
        h0 = orc.encoder(sd, mesh.x).float()
    h = torch.randn(mesh.num_nodes, d, generator=torch.Generator().manual_seed(seed))
    idx = _dirichlet_rows(mesh, mixed)
    h[idx] = h0[idx]
    plan = eng.MeshPlan(md, tile_target=tile_target)
    fmap = eng.FixedPointMap(plan, eng.PackedWeights(sd, dev), h0.to(dev), md.prb_data, getattr(md, "unit_normal_vector", None))
    return fmap, h0, h


def _f64(sd, mesh, h, h0):
    with torch.no_grad():
        return orc.function_forward(_sd64(sd), h.double(), h0.double(), _mesh64(mesh))


CASES = [(n, d) for n in FIXTURES for d in WIDTHS]


@pytest.mark.parametrize("name,d", CASES)
def test_single_f(name, d, dev):
    """One f at a random state on the default tiled plan, on tiles of 32 and 100 nodes and on an untiled plan: <= 2e-6 of the
    float64 oracle; the same call twice gives the same bits."""
    _, mesh = load_case(name)
    mixed = "mixed" in name
    sd = _random(d, mixed)
    for tt in (0, 32, 100, -1):
        fmap, h0, h = _setup(mesh, sd, d, mixed, dev, tile_target=tt)
        assert fmap.plan.tiled == (tt >= 0) and fmap.width == d and fmap.lib.psignn_latent_dim() == d
        want = _f64(sd, mesh, h, h0)
        got = fmap(h.to(dev))
        e = rel_l2(got, want)
        print(f"WIDTH single f {name} d={d} tile_target={tt}: rel-L2 vs fp64 oracle {e:.2e}")
        assert e <= 2e-6, (tt, e)
        assert torch.equal(got, fmap(h.to(dev)))
        if tt >= 0:   # the plan-order entry point is the same function
            assert torch.equal(fmap.from_plan(fmap.fp(fmap.to_plan(h.to(dev)))), got)
        idx = _dirichlet_rows(mesh, mixed)
        assert torch.equal(got.cpu()[idx], h0[idx])


@pytest.mark.parametrize("case,mixed", [("halo512", False), ("jvp682", True)])
def test_single_f_at_the_largest_lds_requests(case, mixed, dev):
    """Width 16 on the plans with the most LDS rows a tiled plan can have: 768 rows x 128 B (dirichlet, 98 304 B) and 682 rows x
    192 B (mixed, 130 944 B).  Both plans must tile; every tile <= 2e-6 of the float64 oracle."""
    eng = pkg("engine")
    d = 16
    c = lg.build(case, mixed)
    sd = _random(d, mixed)
    md = c.mesh.to(dev)
    plan = eng.MeshPlan(md, tile_target=c.tile_target)
    assert c.tiled and plan.tiled and plan.max_tile_rows == c.max_rows
    N = c.mesh.num_nodes
    gen = torch.Generator().manual_seed(21)
    h0, h = (0.3 * torch.randn(N, d, generator=gen) for _ in range(2))
    fmap = eng.FixedPointMap(plan, eng.PackedWeights(sd, dev), h0.to(dev), md.prb_data, getattr(md, "unit_normal_vector", None))
    want = _f64(sd, c.mesh, h, h0)
    got = fmap(h.to(dev))
    e = lg.tile_errors(got, want, plan.export("perm"), plan.export("tile_ptr"))
    print(f"WIDTH limits {case} d={d}: rows {plan.max_tile_rows}, worst tile {e.max():.2e}, whole {rel_l2(got, want):.2e}")
    assert e.max() <= 2e-6, (int(np.argmax(e)), float(e.max()))
    assert torch.equal(got, fmap(h.to(dev)))


@pytest.mark.parametrize("d", WIDTHS)
def test_encoder_decoder_and_mixed_two_group_launch(d, dev, monkeypatch):
    eng, nat = pkg("engine"), pkg("_native")
    _, mesh = load_case("hex13_mixed_s1")
    sd = _random(d, True)
    P = "autoencoder."
    with torch.no_grad():
        h0 = orc.encoder(_sd64(sd), mesh.x.double())
        u = orc.decoder(_sd64(sd), h0)
    enc = eng.mlp2(mesh.x.to(dev), *(sd[P + f"encoder.mlp.mlp.{k}"].to(dev) for k in ("0.weight", "0.bias", "2.weight", "2.bias")))
    dec = eng.mlp2(h0.float().to(dev), *(sd[P + f"decoder.mlp.mlp.{k}"].to(dev) for k in ("0.weight", "0.bias", "2.weight", "2.bias")))
    assert enc.shape == (mesh.num_nodes, d) and rel_l2(enc, h0) < 1e-6 and rel_l2(dec, u) < 1e-6
    # the two-group launch of the mixed family forced at small size: bit-equal to the single launch
    fmap, _, h = _setup(mesh, sd, d, True, dev)
    lib = nat.lib(d)
    monkeypatch.delenv("PSIGNN_MIXED_SPLIT_MIN", raising=False)
    lib.psignn_reload_knobs()
    one = fmap(h.to(dev))
    monkeypatch.setenv("PSIGNN_MIXED_SPLIT_MIN", "1")
    lib.psignn_reload_knobs()
    two = fmap(h.to(dev))
    monkeypatch.delenv("PSIGNN_MIXED_SPLIT_MIN")
    lib.psignn_reload_knobs()
    assert torch.equal(one, two)


@pytest.mark.parametrize("name,d", CASES)
def test_broyden_first_iterations(name, d, dev):
    """Twelve on-device Broyden iterations from h0 against the oracle's solver on the same map (the early-trajectory part of
    test_config2_mixed_100k's comparison); the plan-less solver (solve_callable) runs the same iteration."""
    solver = pkg("utilities.solver")
    _, mesh = load_case(name)
    mixed = "mixed" in name
    sd = _random(d, mixed)
    fmap, h0, _ = _setup(mesh, sd, d, mixed, dev)
    K = 12
    with torch.no_grad():
        ref = orc.broyden(lambda H: orc.function_forward(sd, H, h0, mesh), h0, threshold=K, eps=1e-12)
    out = solver.broyden(fmap, fmap.h0, threshold=K, eps=1e-12, keep_trace=True)
    print(f"WIDTH broyden12 {name} d={d}: rel_trace {[f'{r:.3e}' for r in out['rel_trace'][:K]]} oracle "
          f"{[f'{float(r):.3e}' for r in ref['rel_trace'][:K]]} iterate 3 {rel_l2(out['xest_trace'][3], ref['xest_trace'][3]):.2e}")
    assert out["n_iter"] == K
    np.testing.assert_allclose(out["rel_trace"][:5], [float(r) for r in ref["rel_trace"][:5]], rtol=5e-3)
    assert rel_l2(out["xest_trace"][3], ref["xest_trace"][3]) < 1e-5
    assert out["rel_trace"][K - 1] < 0.2 * out["rel_trace"][0]
    for hist in (torch.bfloat16,):   # the bf16 pair history runs on the same flat kernels: early entries on the fp32 trajectory
        ob = solver.broyden(fmap, fmap.h0, threshold=K, eps=1e-12, keep_trace=False, history_dtype=hist)
        np.testing.assert_allclose(ob["rel_trace"][:2], out["rel_trace"][:2], rtol=5e-3)
    oc = solver.broyden(lambda H: fmap(H), fmap.h0, threshold=K, eps=1e-12, keep_trace=False)
    np.testing.assert_allclose(oc["rel_trace"][:5], [float(r) for r in ref["rel_trace"][:5]], rtol=5e-3)


@pytest.mark.parametrize("name,d", CASES)
def test_converged_solve_through_the_model(name, d, dev):
    """ModelPSIGNN(...).eval() at fw_tol 1e-7: stops below eps without a protective break in at most twice the oracle's float32
    step count, node states and decoded u <= 1e-5 of the oracle's float64 fixed point; the launch record of the width library
    shows the tile kernels and none of the gather kernels."""
    nat = pkg("_native")
    _, mesh = load_case(name)
    mixed = "mixed" in name
    sd = _random(d, mixed)
    net = _mod(mixed).ModelPSIGNN(dict(latent_dim=d, n_layers=1, fw_tol=1e-7, fw_thres=600))
    net.load_state_dict(sd, strict=True)
    net = net.to(dev).eval()
    md = mesh.to(dev)
    torch.set_default_dtype(torch.float64)   # the oracle's solver allocates its pair history in the default dtype
    try:
        with torch.no_grad():
            u64, _, o64 = orc.model_forward(_sd64(sd), _mesh64(mesh), fw_tol=1e-12, fw_thres=600)
    finally:
        torch.set_default_dtype(torch.float32)
    nat.prof_enable(True, width=d)
    nat.prof_collect(width=d)
    try:
        u, loss = net(md)
        _, out = net._solve(md)
        rec = nat.prof_collect(width=d)
    finally:
        nat.prof_enable(False, width=d)
    e_h, e_u = rel_l2(out["result"], o64["result"]), rel_l2(u, u64)
    print(f"WIDTH converged {name} d={d}: nsteps {loss['nsteps']} (oracle fp32 {ORACLE_STEPS[(name, d)]}), lowest {out['lowest']:.2e}, "
          f"node states {e_h:.2e}, u {e_u:.2e}; launches {sorted(rec)}")
    assert out["lowest"] < 1e-7 and not out["prot_break"]
    assert loss["nsteps"] <= 2 * ORACLE_STEPS[(name, d)]
    assert e_h <= 1e-5 and e_u <= 1e-5
    assert engine_plan_is_tiled(md)
    assert rec.get("k_f_tile", (0,))[0] > 0 and rec.get("k_f_tile_fused", (0,))[0] > 0
    assert not any(k.startswith(("k_project", "k_node")) for k in rec), sorted(rec)
    assert torch.equal(net.inference(md), u)
    it = _mod(mixed).ModelPSIGNNIterative(dict(latent_dim=d, n_layers=1, fw_tol=1e-7, fw_thres=600))
    it.load_state_dict(sd, strict=True)
    od = it.to(dev).eval()(md)
    assert od["nstep"] == loss["nsteps"] and len(od["sol_dic"]) >= 2


def engine_plan_is_tiled(md):
    return bool(pkg("engine").plan_for(md).tiled)


@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("mixed", [False, True])
def test_batched_shard(d, mixed, dev):
    """Three maps of one width through broyden_solve_batch: traces, step count and result of each bit-identical to its own
    single-mesh solve with the same solver object."""
    data, eng = pkg("data"), pkg("engine")
    sd = _random(d, mixed)
    net = _mod(mixed).ModelPSIGNN(dict(latent_dim=d, n_layers=1, fw_tol=1e-6, fw_thres=120))
    net.load_state_dict(sd)
    net = net.to(dev).eval()
    meshes = [data.make_hex_problem(n, seed=s, mixed=mixed) for n, s in ((13, 0), (26, 0), (13, 3))]
    mds = [m.to(dev) for m in meshes]
    with torch.no_grad():
        fmaps = [net.deqdss.f.bind(net.autoencoder.encoder(md.x), md) for md in mds]
    assert all(f.plan.tiled and f.width == d for f in fmaps)
    total = sum(f.plan.N for f in fmaps) * d
    solvers = [eng.DeviceBroyden(plan=f.plan, threshold=120, keep_trace=False, shard_elems=total, width=d) for f in fmaps]
    try:
        assert eng.shard_batchable(solvers)
        single = [sv.solve(f, 1e-6) for sv, f in zip(solvers, fmaps)]
        outs = eng.broyden_solve_batch(solvers, fmaps, 1e-6)
        for a, b in zip(single, outs):
            assert a["n_iter"] == b["n_iter"] and a["nstep"] == b["nstep"] and a["stop_reason"] == b["stop_reason"]
            assert a["rel_trace"] == b["rel_trace"] and a["abs_trace"] == b["abs_trace"]
            assert torch.equal(a["result"], b["result"])
            assert a["lowest"] < 1e-6
        # a solver of another width is refused on the host, and never shares a shard
        other = eng.DeviceBroyden(plan=fmaps[0].plan, threshold=120, keep_trace=False, shard_elems=total)
        try:
            assert not eng.shard_batchable([other] + solvers[1:])
            with pytest.raises(pkg("_native").NativeError, match="latent_dim"):
                other.solve(fmaps[0], 1e-6)
        finally:
            other.close()
    finally:
        for sv in solvers:
            sv.close()


@pytest.mark.parametrize("d", WIDTHS)
def test_picard_and_anderson(d, dev):
    """forward_iteration and anderson against the oracle's on the same f, twice.  Once as
    test_forward_iteration_anderson_newton runs them (stop tolerance 1e-5, at most twenty steps) with all of its tolerances.
    Once through all twenty steps (eps 1e-12): step count, result, and at the same relative tolerances every trace entry the
    number format can carry to that tolerance.  An entry is |z' - z| / |z| of float32 iterates, so it holds rounding noise of
    about one float32 ulp, 6e-8, in absolute terms (width 8 passes 1e-7 inside twenty steps and ends at 4.7e-8): it is
    comparable to rtol only while it is above 6e-8 / rtol -- 3e-5 for Picard (rtol 2e-3), 6e-6 for Anderson (rtol 1e-2).  On the
    CPU the oracle's own float32 and float64 runs agree to 4e-5 / 2e-4 on those entries and differ by 3e-3 (Picard, more than
    the tolerance) already on the entries between 1e-6 and 3e-5."""
    solver = pkg("utilities.solver")
    _, mesh = load_case("hex13_dirichlet_s0")
    sd = _random(d, False)
    fmap, h0, _ = _setup(mesh, sd, d, False, dev)
    f_cpu = lambda H: orc.function_forward(sd, H, h0, mesh)
    fl = lambda tr: np.array([float(t) for t in tr])
    for eps in (1e-5, 1e-12):
        with torch.no_grad():
            ref = orc.forward_iteration(f_cpu, h0.clone(), eps=eps, threshold=20)
            refa = orc.anderson(f_cpu, h0.clone(), threshold=20, eps=eps)
        out = solver.forward_iteration(fmap, fmap.h0, eps=eps, threshold=20)
        outa = solver.anderson(fmap, fmap.h0, threshold=20, eps=eps)
        got, want, gota, wanta = fl(out["rel_trace"]), fl(ref["rel_trace"]), fl(outa["rel_trace"]), fl(refa["rel_trace"])
        print(f"WIDTH picard/anderson d={d} eps={eps}: nstep {out['nstep']} / {ref['nstep']}, anderson {outa['nstep']} / {refa['nstep']}; "
              f"last entries {got[-1]:.2e} / {want[-1]:.2e}, {gota[-1]:.2e} / {wanta[-1]:.2e}")
        assert out["nstep"] == ref["nstep"] and len(got) == len(want)
        assert rel_l2(out["result"], ref["result"]) < 1e-5
        assert rel_l2(outa["result"], refa["result"]) < 1e-3
        np.testing.assert_allclose(gota[:5], wanta[:5], rtol=1e-2)
        if eps == 1e-5:
            np.testing.assert_allclose(got, want, rtol=2e-3)
            assert abs(outa["nstep"] - refa["nstep"]) <= 3
        else:
            assert out["nstep"] == 20
            assert len(gota) == len(wanta)      # no early stop: nothing is padded
            keep, keepa = want > 6e-8 / 2e-3, wanta > 6e-8 / 1e-2
            assert keep.sum() >= 5 and keepa.sum() >= 5
            np.testing.assert_allclose(got[keep], want[keep], rtol=2e-3)
            np.testing.assert_allclose(gota[keepa], wanta[keepa], rtol=1e-2)
    assert torch.equal(fmap.from_plan(fmap.picard_p(fmap.to_plan(fmap.h0), 3)), fmap(fmap(fmap(fmap.h0))))


@pytest.mark.parametrize("d", WIDTHS)
def test_two_layer_block(d, dev):
    """n_layers = 2 at widths 8 and 16: one f on the tile kernels and on the gather kernels (layer 1 reads its own weight blocks,
    LayerNorm on the last layer only; the mixed family evaluates its last layer) <= 2e-6 of the float64 oracle, and the first
    Broyden iterations (the unfused route: f per iteration, then the residual kernels) on the oracle's trajectory."""
    solver = pkg("utilities.solver")
    for name in ("hex13_dirichlet_s0", "hex13_mixed_s1"):
        _, mesh = load_case(name)
        mixed = "mixed" in name
        sd = _random(d, mixed, L=2)
        for tt in (0, 100, -1):
            fmap, h0, h = _setup(mesh, sd, d, mixed, dev, tile_target=tt)
            assert fmap.weights.n_layers == 2 and fmap.plan.tiled == (tt >= 0)
            e = rel_l2(fmap(h.to(dev)), _f64(sd, mesh, h, h0))
            print(f"WIDTH two layers {name} d={d} tile_target={tt}: rel-L2 vs fp64 oracle {e:.2e}")
            assert e <= 2e-6, (name, tt, e)
        fmap, h0, _ = _setup(mesh, sd, d, mixed, dev)
        with torch.no_grad():
            ref = orc.broyden(lambda H: orc.function_forward(sd, H, h0, mesh), h0, threshold=6, eps=1e-12)
        out = solver.broyden(fmap, fmap.h0, threshold=6, eps=1e-12, keep_trace=True)
        np.testing.assert_allclose(out["rel_trace"][:5], [float(r) for r in ref["rel_trace"][:5]], rtol=5e-3)
        assert rel_l2(out["xest_trace"][3], ref["xest_trace"][3]) < 1e-5


def _two_widths_child():
    """Body of test_two_widths_in_one_process, run in a process of its own: nothing has loaded a width library before."""
    eng, mp, nat = pkg("engine"), pkg("model_psignn"), pkg("_native")
    dev = torch.device("cuda:0")
    _, mesh = load_case("hex13_dirichlet_s0")
    md = mesh.to(dev)
    cfg = dict(n_layers=1, fw_tol=1e-6, fw_thres=300)
    n10 = mp.ModelPSIGNN(dict(cfg, latent_dim=10))
    n10.load_state_dict(load_weights("dirichlet"))
    n10 = n10.to(dev).eval()
    u10, l10 = n10(md)
    assert list(nat._libs) == [10], list(nat._libs)      # taken before the width-16 library was ever loaded
    plan = eng.plan_for(md)
    n16 = mp.ModelPSIGNN(dict(cfg, latent_dim=16))
    n16.load_state_dict(_random(16, False))
    n16 = n16.to(dev).eval()
    u16, l16 = n16(md)
    assert 16 in nat._libs and eng.plan_for(md) is plan  # the plan is width-free: both models share it
    for _ in range(2):
        a, la = n10(md)
        b, lb = n16(md)
        assert torch.equal(a, u10) and la["nsteps"] == l10["nsteps"]
        assert torch.equal(b, u16) and lb["nsteps"] == l16["nsteps"]
    # a map refuses a state, an h_initial or a solver of another width on the host
    f16 = n16.deqdss.f.bind(n16.autoencoder.encoder(md.x), md)
    f10 = n10.deqdss.f.bind(n10.autoencoder.encoder(md.x), md)
    with pytest.raises(nat.NativeError):
        f16(f10.h0)
    with pytest.raises(nat.NativeError):
        eng.FixedPointMap(plan, f16.weights, f10.h0, md.prb_data)
    sv = eng.DeviceBroyden(plan=plan, threshold=5)
    with pytest.raises(nat.NativeError, match="latent_dim"):
        sv.solve(f16, 1e-3)
    sv.close()
    print("TWO_WIDTHS_OK nsteps", l10["nsteps"], l16["nsteps"])


def test_two_widths_in_one_process(dev):
    """A width-10 model (shipped dirichlet checkpoint) and a width-16 model called alternately in a fresh process: the width-10
    outputs are bit-identical to the ones taken before the width-16 library was loaded, and one MeshPlan serves both."""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    code = (f"import sys; sys.path.insert(0, {here!r}); import conftest; "
            "import test_gpu_latent_width as t; t._two_widths_child()")
    r = subprocess.run([sys.executable, "-c", code], cwd=os.path.dirname(here), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "TWO_WIDTHS_OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def test_derivatives_are_refused_on_the_host(dev):
    """At width 16 every derivative entry of a map, the Newton solvers and ModelDEQDSS.forward raise the "forward inference
    only" error before any native call."""
    nat, solver, eng = pkg("_native"), pkg("utilities.solver"), pkg("engine")
    _, mesh = load_case("hex13_dirichlet_s0")
    sd = _random(16, False)
    fmap, h0, h = _setup(mesh, sd, 16, False, dev)
    H, V = h.to(dev), torch.ones_like(h).to(dev)
    calls = [lambda: fmap.jvp(H, V), lambda: fmap.jvp_p(H, V), lambda: fmap.vjp(H, V), lambda: fmap.vjp_p(H, V),
             lambda: fmap.linearize_p(H), lambda: fmap.param_vjp(H, V), lambda: fmap.param_vjp_p(H, V),
             lambda: fmap.param_vjp_init(H, V), lambda: fmap.vjp_backward(H, V, V), lambda: fmap.vjp_backward_p(H, V, V),
             lambda: eng.Linearization(fmap), lambda: solver.newton(fmap, fmap.h0), lambda: solver.newton_krylov(fmap, fmap.h0)]
    for c in calls:
        with pytest.raises(nat.NativeError, match="forward inference only"):
            c()
    assert not fmap.can_linearize() and not fmap.can_tile_vjp_backward()
    net = pkg("model_psignn").ModelDEQDSS(dict(latent_dim=16, n_layers=1, fw_tol=1e-6, fw_thres=100))
    net.load_state_dict(sd)
    net = net.to(dev)
    md = mesh.to(dev)
    for mode in (net.train(), net.eval()):
        with pytest.raises(nat.NativeError, match="forward inference only"):
            mode(md)
    u = net.eval().inference(md)
    assert u.shape == (mesh.num_nodes, 1) and torch.isfinite(u).all()
    assert len(net.iterative_inference(md)["sol_dic"]) >= 2
