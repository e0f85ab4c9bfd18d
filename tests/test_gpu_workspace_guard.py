"""No entry point reaches past the workspace its size query promises (csrc/workspace.h), and none depends on having more.

Every public entry point that takes a caller workspace is called twice on small meshes: once with a workspace of EXACTLY the
queried size, embedded in an owned buffer about three times as large whose two other parts hold a fixed bit pattern, and once
with a plain workspace of more than twice the size.  The guard parts must be untouched and the two results bit-identical.  All of
it is owned memory: a layout that overruns its declared size shows as a changed guard word, not as a fault.

Cases: the smallest golden mesh of each family (547 nodes -- not a multiple of 64, more than one tile), a 487-node mesh, and untiled
plans (tile_target = -1) of both families, so that the gather paths run; n_layers 1 and 2 where the entry point supports it."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_case, load_weights, pkg

pytestmark = pytest.mark.gpu

PATTERN = 0x5A5A5A5A
CASES = [("hex13_dirichlet_s0", 0), ("hex13_mixed_s1", 0), ("original_dirichlet_s0", 0), ("hex13_dirichlet_s0", -1), ("hex13_mixed_s1", -1)]


def _guarded(n, dev):
    """(whole buffer, its middle part of exactly n floats, offset of that part); the part starts on a 256-byte boundary like a
    buffer of its own would."""
    lead = (n + 63) // 64 * 64
    buf = torch.full((lead + 2 * n,), PATTERN, dtype=torch.int32, device=dev)
    mid = buf[lead:lead + n]
    mid.zero_()
    return buf, mid.view(torch.float32), lead


def _intact(buf, lead, n):
    return bool((buf[:lead] == PATTERN).all()) and bool((buf[lead + n:] == PATTERN).all())


def _same(a, b):
    if torch.is_tensor(a):
        return torch.equal(a, b)
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a is None and b is None or a == b


def _twice(owner, attr, n, call, dev, what):
    """call() with owner.<attr> = a guarded workspace of n floats, then with a plain one of 2 n + 4096."""
    n = int(n)
    buf, mid, lead = _guarded(n, dev)
    setattr(owner, attr, mid)
    first = call()
    torch.cuda.synchronize()
    assert getattr(owner, attr) is mid, f"{what}: the call replaced the workspace of the queried size ({n} floats)"
    assert _intact(buf, lead, n), f"{what}: wrote outside its workspace of {n} floats"
    setattr(owner, attr, torch.zeros(2 * n + 4096, dtype=torch.float32, device=dev))
    second = call()
    assert _same(first, second), f"{what}: the result depends on the size of the workspace"
    setattr(owner, attr, None)


def _block_weights(family, L):
    if family == "dirichlet":
        sd = load_weights("dirichlet")
        out = dict(sd)
        for k, t in sd.items():
            for mod in ("phi_to_list", "phi_from_list", "update_list"):
                if f".f.{mod}.0." in k:
                    for l in range(1, L):
                        out[k.replace(f"{mod}.0.", f"{mod}.{l}.")] = t.clone()
        return out
    if L == 1:
        return load_weights("mixed")
    torch.manual_seed(6)
    net = pkg("mixed").ModelPSIGNN(dict(latent_dim=10, n_layers=L))
    return {k: v.detach().clone() for k, v in net.state_dict().items()}


@pytest.mark.parametrize("L", [1, 2])
@pytest.mark.parametrize("name,tt", CASES)
def test_f_and_its_derivatives_stay_inside_their_workspaces(name, tt, L, dev):
    eng, nat = pkg("engine"), pkg("_native")
    lib = nat.lib()
    mixed = "mixed" in name
    _, mesh = load_case(name)
    md = mesh.to(dev)
    plan = eng.MeshPlan(md, tile_target=tt)
    assert bool(plan.tiled) == (tt == 0) and plan.N % 64 != 0
    gen = torch.Generator().manual_seed(3)
    h0, h, v, g = (torch.randn(plan.N, 10, generator=gen).to(dev) for _ in range(4))
    fm = eng.FixedPointMap(plan, eng.PackedWeights(_block_weights("mixed" if mixed else "dirichlet", L), dev), h0, md.prb_data,
                           md.unit_normal_vector if mixed else None)
    hd = plan.handle
    layers = int(lib.psignn_f_layers_workspace_floats(hd, L))
    nf = int(lib.psignn_f_workspace_floats(hd))
    npv = int(lib.psignn_f_param_vjp_workspace_floats(hd)) + layers
    njr = int(lib.psignn_f_vjp_backward_workspace_floats(hd)) + layers
    hp, vp, gp = fm.to_plan(h), fm.to_plan(v), fm.to_plan(g)
    fm.fp(hp)   # the map's plan-order copies of h_initial / prb / normals
    _twice(plan, "_work", nf, lambda: fm(h), dev, "psignn_f_forward")
    _twice(plan, "_work", nf, lambda: fm.fp(hp), dev, "psignn_f_forward_p")
    _twice(plan, "_work", nf + layers, lambda: fm.jvp(h, v), dev, "psignn_f_jvp")
    if plan.tiled:
        _twice(plan, "_work", nf + layers, lambda: fm.jvp_p(hp, vp), dev, "psignn_f_jvp_p / _pw")
    _twice(plan, "_work", nf + layers, lambda: fm.vjp(h, v), dev, "psignn_f_vjp")
    _twice(plan, "_work", nf + layers, lambda: fm.vjp_p(hp, vp), dev, "psignn_f_vjp_p")
    _twice(plan, "_pwork", npv, lambda: fm.param_vjp_init(h, v), dev, "psignn_f_param_vjp_ex")
    if plan.tiled and not mixed:
        _twice(plan, "_pwork", npv, lambda: fm.param_vjp_p(hp, vp), dev, "psignn_f_param_vjp_p")
    _twice(plan, "_jwork", njr, lambda: fm.vjp_backward(h, v, g), dev, "psignn_f_vjp_backward")
    if fm.can_tile_vjp_backward():
        _twice(plan, "_jwork", lib.psignn_f_vjp_backward_p_workspace_floats(hd), lambda: fm.vjp_backward_p(hp, vp, gp), dev,
               "psignn_f_vjp_backward_p")
    else:
        assert L > 1 or mixed or not plan.tiled
    # the GMRES adjoint solve: a few cycles of a short restart length at a state that is no fixed point (the products are what matter)
    gm = eng.DeviceGmres(plan.N * 10, dev, 4)
    gm._work_key = (plan, L)

    def adjoint():
        r = gm.solve_adjoint(fm, h, g, 1e-6, 10)
        return r["result"], r["nstep"], r["rel_trace"]
    _twice(gm, "_work", lib.psignn_gmres_adjoint_workspace_floats(hd, L), adjoint, dev, "psignn_gmres_solve_adjoint")
    gm._work_key = None
    gm.close()


@pytest.mark.parametrize("name,tt", CASES)
def test_dsgps_step_backward_and_forward_stay_inside_their_workspaces(name, tt, dev):
    eng, nat = pkg("engine"), pkg("_native")
    lib = nat.lib()
    mixed = "mixed" in name
    w = np.load(os.path.join(GOLDEN, "weights_dsgps_mixed.npz" if mixed else "weights_dsgps.npz"))
    sd = {n: torch.from_numpy(w[n]) for n in w.files if n != "k"}
    _, mesh = load_case(name)
    md = mesh.to(dev)
    plan = eng.MeshPlan(md, tile_target=tt)
    gen = torch.Generator().manual_seed(5)
    h0, h, wv = (torch.randn(plan.N, 10, generator=gen).to(dev) for _ in range(3))
    nrm = md.unit_normal_vector if mixed else None
    wf, wg = eng.pack_dsgps_train(sd, dev)
    _twice(plan, "_dswork", lib.psignn_dsgps_step_backward_workspace_floats(plan.handle),
           lambda: eng.dsgps_step_backward(plan, wf, wg, h, md.prb_data, wv, nrm), dev, "psignn_dsgps_step_backward")
    if not plan.tiled:
        return   # the forward kernels need a tiled plan
    packed = eng.pack_dsgps(sd, dev)
    prb = md.prb_data.float().contiguous()
    holder = type("W", (), {})()

    def forward():
        out = torch.empty_like(h0)
        with torch.cuda.device(dev):
            nat.check(lib.psignn_dsgps_forward(plan.handle, nat.ptr(packed), 3, nat.ptr(h0), nat.ptr(prb),
                                               nat.ptr(None if nrm is None else nrm.float().contiguous()), nat.ptr(out), nat.ptr(holder.work),
                                               nat.stream_ptr(dev)), "psignn_dsgps_forward")
        return out
    _twice(holder, "work", 4 * plan.N * 10, forward, dev, "psignn_dsgps_forward")
    hp, h0p, prbp = plan.permute(h, True), plan.permute(h0, True), plan.permute(prb, True)
    nrmp = None if nrm is None else plan.permute(nrm.float(), True)
    a, b = eng.dsgps_step_p(plan, packed, hp, h0p, prbp, nrmp), eng.dsgps_step_p(plan, packed, hp, h0p, prbp, nrmp)
    assert torch.equal(a, b)   # the step takes no workspace: it only has to agree with itself


def test_dss_and_mlp2_stay_inside_their_workspaces(dev):
    eng, nat, dss = pkg("engine"), pkg("_native"), pkg("dss")
    lib = nat.lib()
    w = np.load(os.path.join(GOLDEN, "weights_dss.npz"))
    sd = {n: torch.from_numpy(w[n]) for n in w.files if n not in ("k", "alpha")}
    alpha = float(w["alpha"])
    _, mesh = load_case("hex13_dirichlet_s0")
    batch = dss.to_dss_batch(mesh).to(dev)
    holder = type("W", (), {})()
    gen = torch.Generator().manual_seed(7)
    # the plan of the DSS graph: the scalar edge feature rides in the third edge_attr column (dss.DeepStatisticalSolver._plan)
    a_ij, a_norm = dss.DeepStatisticalSolver._fields(batch)
    ea = torch.cat([torch.zeros((a_norm.shape[0], 2), device=dev), a_norm.reshape(-1, 1).float()], dim=1).contiguous()
    view = pkg("data").MeshData(x=batch.x, edge_index=batch.edge_index, a_ij=a_ij, edge_attr=ea,
                                tags=torch.zeros((batch.x.shape[0], 1), device=dev), pos=batch.pos)
    for tt in (0, -1):
        plan = eng.MeshPlan(view, tile_target=tt)
        h, wv = (torch.randn(plan.N, 10, generator=gen).to(dev) for _ in range(2))
        wf = eng.pack_dss_train(sd, 1, dev)
        _twice(plan, "_dsswork", lib.psignn_dss_step_backward_workspace_floats(plan.handle),
               lambda: eng.dss_step_backward(plan, wf, 1, alpha, h, batch.b_prime_norm, wv), dev, "psignn_dss_step_backward")
        if not plan.tiled:
            continue
        packed = eng.pack_dss(sd, 3, dev)
        bp = batch.b_prime_norm.float().contiguous()

        def forward():
            out = torch.empty((plan.N, 10), dtype=torch.float32, device=dev)
            with torch.cuda.device(dev):
                nat.check(lib.psignn_dss_forward(plan.handle, nat.ptr(packed), 3, alpha, nat.ptr(bp), nat.ptr(out), nat.ptr(holder.work),
                                                 nat.stream_ptr(dev)), "psignn_dss_forward")
            return out
        _twice(holder, "work", 23 * plan.N, forward, dev, "psignn_dss_forward")
        a = eng.dss_step_p(plan, packed, 1, alpha, plan.permute(h, True), plan.permute(bp, True))
        assert torch.equal(a, eng.dss_step_p(plan, packed, 1, alpha, plan.permute(h, True), plan.permute(bp, True)))
    # backward of the two-layer MLP: lengths around the wave and block sizes of the reduction
    for n in (1, 65, 547):
        x, gy = torch.randn(n, 3, generator=gen).to(dev), torch.randn(n, 2, generator=gen).to(dev)
        w1, b1, w2 = (torch.randn(s, generator=gen).to(dev) for s in ((10, 3), (10,), (2, 10)))

        def backward():
            gx = torch.empty_like(x)
            gflat = torch.empty(10 * 3 + 10 + 2 * 10 + 2, dtype=torch.float32, device=dev)
            with torch.cuda.device(dev):
                nat.check(lib.psignn_mlp2_backward(nat.ptr(x), nat.ptr(gy), n, 3, 10, 2, nat.ptr(w1), nat.ptr(b1), nat.ptr(w2), nat.ptr(gx),
                                                   nat.ptr(gflat), nat.ptr(holder.work), nat.stream_ptr(dev)), "psignn_mlp2_backward")
            return gx, gflat
        _twice(holder, "work", lib.psignn_mlp2_backward_workspace_floats(n), backward, dev, "psignn_mlp2_backward")
