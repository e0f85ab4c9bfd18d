"""The graphs, states and probes of tests/test_gpu_f64_vjp_backward.py, shared with scripts/calib_f64_vjp_backward.py so that the
gates are measured on exactly what the test runs.  Everything here is CPU float64; nothing touches a device."""
from dataclasses import dataclass

import numpy as np
import torch

import limit_graphs as lg
from conftest import CASES, load_case, load_weights, pkg
from oracle import psignn_oracle as orc

FIXTURES = ["hex13_dirichlet_s0", "hex13_mixed_s1", "original_dirichlet_s0"]
LIMITS = ["slots255_split", "ragged65", "slots256"]
LINES = [1, 127, 128, 129]
CHUNK = 128   # rows per partial of the parameter sums (psignn_f64_param_vjp_chunk_rows)


@dataclass
class VBCase:
    name: str
    sd: dict          # float32 state dict
    mesh: object      # MeshData (CPU, float32)
    H: torch.Tensor   # (N, 10) float64
    h0: object        # (N, 10) float64, or None: the float64 encoder's output
    V: torch.Tensor
    Gbar: torch.Tensor
    tile_target: int = 0
    tiled: object = None   # expected outcome of the tile builder (None: not part of the case)
    limits: bool = False   # a structure-limit graph: J^T V has the wider gates of tests/test_gpu_f64_deriv.py


def randn(shape, seed, scale=1.0):
    return scale * torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def to64(sd, mesh):
    m64 = mesh.clone()
    for k, v in list(vars(mesh).items()):
        if torch.is_tensor(v) and v.is_floating_point():
            setattr(m64, k, v.double())
    return {k: v.double() for k, v in sd.items()}, m64


def encoded(sd, mesh):
    s64, m64 = to64(sd, mesh)
    with torch.no_grad():
        return orc.encoder(s64, m64.x)


def line_graph(N, mixed):
    """A chain 0 - 1 - ... - N-1 of mirror pairs plus one self loop per node, edges shuffled.  Node 0 is never a boundary node (N = 1
    is one live row with its self loop); every seventh node is Dirichlet and, on mixed graphs, every fifth a Neumann node."""
    rng = np.random.default_rng(500 + N + (7 if mixed else 0))
    src, dst, attr = list(range(N)), list(range(N)), [np.zeros(3, np.float32)] * N
    for u in range(N - 1):
        a = rng.standard_normal(3).astype(np.float32)
        src += [u, u + 1]
        dst += [u + 1, u]
        attr += [a, a * lg.MIRROR]
    order = rng.permutation(len(src))
    ei = np.stack([np.asarray(src), np.asarray(dst)])[:, order].astype(np.int64)
    ea = np.stack(attr)[order]
    kind = np.zeros(N, np.int64)
    kind[3::7] = 1
    if mixed:
        kind[2::5] = 2
        tags = np.eye(3, dtype=np.float32)[kind]
    else:
        tags = kind.reshape(-1, 1).astype(np.float32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    m = pkg("data").MeshData(x=t(rng.standard_normal((N, 1)).astype(np.float32)), edge_index=t(ei), edge_attr=t(ea),
                             a_ij=t(rng.standard_normal((ei.shape[1], 1)).astype(np.float32)),
                             y=t(rng.standard_normal((N, 1)).astype(np.float32)), sol=torch.zeros(N, 1),
                             prb_data=t(rng.standard_normal((N, 3 if mixed else 2)).astype(np.float32)), tags=t(tags), pos=None)
    if mixed:
        nv = rng.standard_normal((N, 2)).astype(np.float32)
        m.unit_normal_vector = t(nv / np.linalg.norm(nv, axis=1, keepdims=True))
    return m


def _two_layer(mixed, seed=5):
    torch.manual_seed(seed)
    net = pkg("mixed" if mixed else "model_psignn").ModelPSIGNN(dict(latent_dim=10, n_layers=2))
    for q in net.parameters():
        if q.dim() == 1:
            torch.nn.init.normal_(q, std=0.1)
    return {k: v.detach().clone() for k, v in net.state_dict().items()}


_hex60 = {}


def hex60(mixed):
    if mixed not in _hex60:
        mesh = pkg("data").make_hex_problem(60, seed=3, mixed=mixed, compute_sol=False)
        assert mesh.num_nodes == 10981
        sd = load_weights("mixed" if mixed else "dirichlet")
        _hex60[mixed] = (sd, mesh, encoded(sd, mesh))
    return _hex60[mixed]


def probe_rows(N):
    return [CHUNK - 1, CHUNK, CHUNK + 1, N - 1]


def _fam(mixed):
    return "mixed" if mixed else "dirichlet"


def _random_state(N, seed):
    gen = torch.Generator().manual_seed(seed)
    H = 0.3 * torch.randn(N, 10, generator=gen, dtype=torch.float64)
    H0 = 0.3 * torch.randn(N, 10, generator=gen, dtype=torch.float64)
    return H, H0


def _builders():
    b = {}
    for name in FIXTURES:
        for at in ("h0", "fp64_result"):
            def fixture(name=name, at=at):
                g, mesh = load_case(name)
                sd = load_weights(CASES[name])
                h0 = encoded(sd, mesh)
                H = h0 if at == "h0" else torch.from_numpy(g["fp64_result"])
                return VBCase(f"{name}@{at}", sd, mesh, H, None, randn(H.shape, 31), randn(H.shape, 37))
            b[f"{name}@{at}"] = fixture
    for case in LIMITS:
        for mixed in (False, True):
            def limit(case=case, mixed=mixed):
                c = lg.build(case, mixed)
                H, H0 = _random_state(c.mesh.num_nodes, 21)
                return VBCase(f"{case}-{_fam(mixed)}", load_weights(_fam(mixed)), c.mesh, H, H0, randn(H.shape, 31),
                              randn(H.shape, 37), c.tile_target, c.tiled, True)
            b[f"{case}-{_fam(mixed)}"] = limit
    for mixed in (False, True):
        def two(mixed=mixed):
            _, mesh = load_case("hex13_mixed_s1" if mixed else "hex13_dirichlet_s0")
            H, H0 = _random_state(mesh.num_nodes, 22)
            return VBCase(f"two_layers-{_fam(mixed)}", _two_layer(mixed), mesh, H, H0, randn(H.shape, 31), randn(H.shape, 37))
        b[f"two_layers-{_fam(mixed)}"] = two
    for mixed in (False, True):
        for probe in (False, True):
            def big(mixed=mixed, probe=probe):
                sd, mesh, h0 = hex60(mixed)
                V = randn(h0.shape, 31)
                if probe:
                    rows = probe_rows(mesh.num_nodes)
                    sparse = torch.zeros_like(V)
                    sparse[rows] = V[rows]
                    V = sparse
                return VBCase(f"hex60-{_fam(mixed)}-{'probe' if probe else 'dense'}", sd, mesh, h0, None, V, randn(h0.shape, 37))
            b[f"hex60-{_fam(mixed)}-{'probe' if probe else 'dense'}"] = big
    for N in LINES:
        for mixed in (False, True):
            def line(N=N, mixed=mixed):
                H, H0 = _random_state(N, 23)
                return VBCase(f"line{N}-{_fam(mixed)}", load_weights(_fam(mixed)), line_graph(N, mixed), H, H0, randn(H.shape, 31),
                              randn(H.shape, 37))
            b[f"line{N}-{_fam(mixed)}"] = line
    return b


BUILDERS = _builders()
NAMES = list(BUILDERS)


def make(name) -> VBCase:
    return BUILDERS[name]()


def oracle(c: VBCase, V=None, Gbar=None):
    """``orc.function_vjp_backward`` in float64 at the case's state: ({name: grad}, dH, J^T V).  The caller switches torch's default
    dtype to float64 around it where the process default is float32."""
    s64, m64 = to64(c.sd, c.mesh)
    h0 = encoded(c.sd, c.mesh) if c.h0 is None else c.h0
    return orc.function_vjp_backward(s64, c.H.clone(), h0, m64, c.V if V is None else V, c.Gbar if Gbar is None else Gbar)


def _rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    d = float(b.norm())
    return float((a - b).norm()) / d if d > 0 else float((a - b).norm())


def identity_defects(vjp_backward, a, b):
    """The defects of the two exact identities for a callable ``Gbar -> (grads, dH, J^T V)``: the symmetry of the Hessian,
    |<a, dH(b)> - <b, dH(a)>| / (|a| |dH(b)|), and the linearity in Gbar, worst relative L2 of out(a + 2 b) - (out(a) + 2 out(b)) over
    the parameter tensors and of dH.  The test applies the same function to the device."""
    ga, da, _ = vjp_backward(a)
    gb, db, _ = vjp_backward(b)
    gc, dc, _ = vjp_backward(a + 2 * b)
    sym = abs(float((a * db).sum()) - float((b * da).sum())) / (float(a.norm()) * float(db.norm()))
    lin_p = max(_rel(ga[k] + 2 * gb[k], gc[k]) for k in gc)
    lin_h = _rel(da + 2 * db, dc)
    return sym, lin_p, lin_h
