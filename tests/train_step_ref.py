"""The training step of tests/test_gpu_f64_train_step.py and tests/test_host_f64_train_step.py restated on the CPU, with the graphs the
residual tests run on, shared with scripts/calib_f64_train_step.py so that the gates are measured on exactly what the tests run.
Everything here is CPU; nothing touches a device.

``train_step_ref`` is ``orc.training_step`` with both solves taken out: the state ``h*``, the adjoint solution ``y`` and the probe are
handed in and the backward hook returns the given ``y``.  At the oracle's own ``out_fw["result"]`` / ``out_bw["result"]`` it builds the
same autograd graph, so it reproduces the oracle's losses and gradients; at any other ``(h*, y)`` it is what ``loss.backward()``
would leave had the solves ended there.  It takes a dtype, so the same code gives the float32 oracle's value."""
import contextlib

import numpy as np
import torch

import limit_graphs as lg
import vjp_backward_cases as vb
from conftest import CASES, load_case, load_weights, pkg
from oracle import psignn_oracle as orc

FIXTURES = vb.FIXTURES
LIMITS = vb.LIMITS
LINES = [1, 2, 64, 65, 129]
LOSS_KEYS = ["residual_loss", "encoder_loss", "autoencoder_loss", "mse_loss", "mse_dirichlet", "jacobian_loss"]
TWO_LAYER_STEPS = 40   # forward and adjoint iterations of the two-layer cases: the chain, not a fixed point


@contextlib.contextmanager
def default_dtype(dtype):
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        yield
    finally:
        torch.set_default_dtype(old)


def as_dtype(sd, mesh, dtype):
    m = mesh.clone()
    for k, v in list(vars(mesh).items()):
        if torch.is_tensor(v) and v.is_floating_point():
            setattr(m, k, v.to(dtype))
    return {k: v.to(dtype) for k, v in sd.items()}, m


def rel(a, b):
    return vb._rel(a, b)


def train_step_ref(sd, mesh, h_star, y, probe=None, jac_weight=0.0, dtype=torch.float64):
    """(loss, loss_dic, {state-dict name: grad}, grad_h): ``orc.training_step`` at a given state.  ``grad_h``: the cotangent the backward
    hook receives; the hook returns ``y``."""
    s, m = as_dtype(sd, mesh, dtype)
    mse = torch.nn.functional.mse_loss
    with default_dtype(dtype):
        p = {k: t.detach().clone().requires_grad_(True) for k, t in s.items()}
        h_init = orc.encoder(p, m.x)
        H_star = h_star.detach().to(dtype).clone().requires_grad_()
        new_H = orc.function_forward(p, H_star, h_init, m)
        jac_loss = torch.zeros(())
        if probe is not None:
            vJ = torch.autograd.grad(new_H, H_star, probe.to(dtype), retain_graph=True, create_graph=True)[0]
            jac_loss = vJ.norm() ** 2 / H_star.numel()
        seen = {}

        def backward_hook(grad):
            seen["grad_h"] = grad.detach().clone()
            return y.detach().to(dtype)

        new_H.register_hook(backward_hook)
        u = orc.decoder(p, new_H)
        loss_dic = {"residual_loss": orc.residual_loss(u, m)}
        u_d, h_d = u.detach(), new_H.detach()
        loss_dic["encoder_loss"] = mse(orc.encoder(p, u_d), h_d)
        loss_dic["autoencoder_loss"] = mse(orc.decoder(p, orc.encoder(p, u_d).detach()), u_d)
        loss_dic["mse_loss"] = mse(u, m.sol)
        idx = torch.where(m.tags == 1)[0]
        loss_dic["mse_dirichlet"] = mse(u[idx, :], m.x[idx, :])
        loss_dic["jacobian_loss"] = jac_loss
        loss = loss_dic["residual_loss"] + jac_weight * jac_loss + loss_dic["encoder_loss"] + loss_dic["autoencoder_loss"]
        loss.backward()
    grads = {k: (t.grad if t.grad is not None else torch.zeros_like(t)) for k, t in p.items()}
    return loss.detach(), {k: v.detach() for k, v in loss_dic.items()}, grads, seen["grad_h"]


def oracle_step(sd, mesh, probe, fw=(1e-11, 1000), bw=(1e-11, 800), jac_weight=1.0):
    """``orc.training_step`` in float64: (loss, loss_dic, grads, out_fw, out_bw)."""
    s64, m64 = as_dtype(sd, mesh, torch.float64)
    with default_dtype(torch.float64):
        return orc.training_step(s64, m64, fw_tol=fw[0], fw_thres=fw[1], bw_tol=bw[0], bw_thres=bw[1], jac_weight=jac_weight,
                                 probe=probe.double())


def probe_of(N, seed=3):
    return vb.randn((N, 10), seed)


# ------------------------------------------------------------------------------------------------ the cases of the step
def step_case(name):
    """(state dict, mesh, (fw tolerance, steps), (bw tolerance, steps)) of a fixture or of ``two_layers-<family>``."""
    if name in FIXTURES:
        _, mesh = load_case(name)
        return load_weights(CASES[name]), mesh, (1e-11, 1000), (1e-11, 800)
    mixed = name == "two_layers-mixed"
    _, mesh = load_case("hex13_mixed_s1" if mixed else "hex13_dirichlet_s0")
    return vb._two_layer(mixed), mesh, (1e-11, TWO_LAYER_STEPS), (1e-11, TWO_LAYER_STEPS)


STEP_NAMES = FIXTURES + ["two_layers-dirichlet", "two_layers-mixed"]
_steps = {}


def oracle_at(name):
    """The oracle's float64 step of a case, made once: dict with sd, mesh, probe, loss, loss_dic, grads, fw, bw."""
    if name not in _steps:
        sd, mesh, fw, bw = step_case(name)
        probe = probe_of(mesh.num_nodes)
        loss, dic, grads, out_fw, out_bw = oracle_step(sd, mesh, probe, fw, bw)
        _steps[name] = dict(sd=sd, mesh=mesh, probe=probe, loss=loss, loss_dic=dic, grads=grads, fw=out_fw, bw=out_bw)
    return _steps[name]


# ------------------------------------------------------------------------------------------------ the graphs of the residual
def odd_graph():
    """Seven nodes: duplicate edges (0 -> 1 three times, the self loop of 2 twice), one-directional edges (3 -> 4, 5 -> 0), node 6 without
    a self loop, node 4 with nothing but its self loop and one in-edge."""
    src = [0, 0, 0, 1, 2, 2, 3, 5, 0, 1, 3, 4, 5, 6, 2, 6]
    dst = [1, 1, 1, 0, 2, 2, 4, 0, 0, 1, 3, 4, 5, 2, 6, 5]
    rng = np.random.default_rng(77)
    E, N = len(src), 7
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    return pkg("data").MeshData(x=t(rng.standard_normal((N, 1)).astype(np.float32)), edge_index=t(np.array([src, dst], dtype=np.int64)),
                                edge_attr=t(rng.standard_normal((E, 3)).astype(np.float32)),
                                a_ij=t(rng.standard_normal((E, 1)).astype(np.float32)), y=t(rng.standard_normal((N, 1)).astype(np.float32)),
                                sol=torch.zeros(N, 1), prb_data=t(rng.standard_normal((N, 2)).astype(np.float32)),
                                tags=torch.zeros(N, 1), pos=None)


def _residual_builders():
    b = {}
    for name in FIXTURES:
        b[name] = lambda name=name: (load_case(name)[1], 0)
    for case in LIMITS:
        for mixed in (False, True):
            def limit(case=case, mixed=mixed):
                c = lg.build(case, mixed)
                return c.mesh, c.tile_target
            b[f"{case}-{vb._fam(mixed)}"] = limit
    for N in LINES:
        b[f"line{N}"] = lambda N=N: (vb.line_graph(N, False), 0)
    b["odd_graph"] = lambda: (odd_graph(), 0)
    b["hex60"] = lambda: (vb.hex60(False)[1], 0)
    return b


RESIDUAL_BUILDERS = _residual_builders()
RESIDUAL_NAMES = list(RESIDUAL_BUILDERS)


def residual_case(name):
    """(mesh, tile_target, u, w): the graph and two seeded float64 columns."""
    mesh, tile_target = RESIDUAL_BUILDERS[name]()
    N = mesh.num_nodes
    return mesh, tile_target, vb.randn((N, 1), 61), vb.randn((N, 1), 62)


def residual_ref(edge_index, a_ij, u, y):
    """``A u - y`` as ``orc.residual_loss`` forms it (index_add_ over the edge list), in the dtype of ``u``."""
    r, c = edge_index[0], edge_index[1]
    Au = torch.zeros_like(u)
    Au.index_add_(0, r, a_ij.reshape(-1, 1).to(u.dtype) * u.index_select(0, c))
    return Au - y.to(u.dtype)


def residual_t_ref(edge_index, a_ij, r):
    """``A^T r`` in the same form: what autograd sends back through the index_add_."""
    rows, cols = edge_index[0], edge_index[1]
    out = torch.zeros_like(r)
    out.index_add_(0, cols, a_ij.reshape(-1, 1).to(r.dtype) * r.index_select(0, rows))
    return out


# ------------------------------------------------------------------------------------------------ reordering (calibration)
def permuted(mesh, rows, seed, nodes):
    """The same problem with the edge list in another order, or (nodes) with the nodes renumbered: the mesh, the per-node arrays in
    ``rows`` in its numbering, and the map back (None when the numbering is unchanged).  Arrays are told apart by their first
    dimension, so a graph with as many edges as nodes is left alone by the caller."""
    gen = torch.Generator().manual_seed(seed)
    m = mesh.clone()
    N, E = mesh.num_nodes, mesh.edge_index.shape[1]
    assert E != N
    if not nodes:
        pe = torch.randperm(E, generator=gen)
        for k, v in list(vars(mesh).items()):
            if torch.is_tensor(v) and v.dim() >= 1 and v.shape[0] == E and k != "edge_index":
                setattr(m, k, v[pe])
        m.edge_index = mesh.edge_index[:, pe]
        return m, rows, None
    pn = torch.randperm(N, generator=gen)   # new row i is old row pn[i]
    inv = torch.empty_like(pn)
    inv[pn] = torch.arange(N)
    for k, v in list(vars(mesh).items()):
        if torch.is_tensor(v) and v.dim() >= 1 and v.shape[0] == N and k != "edge_index":
            setattr(m, k, v[pn])
    m.edge_index = inv[mesh.edge_index]
    return m, [r[pn] for r in rows], inv


def tensor_class(name, t):
    """The class a gradient tensor's gate belongs to: the autoencoder's MLPs, the matrices of f, the vectors / scalars of f."""
    if name.startswith("autoencoder."):
        return "mlp"
    return "matrix" if t.dim() == 2 and t.shape[0] > 1 else "vector"
