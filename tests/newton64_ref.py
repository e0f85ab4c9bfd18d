"""Torch restatement of the shifted linear solve of the float64 Newton-Krylov solver (csrc/krylov_f64.hip,
``psignn_gmres64_solve_shifted``) and the CPU problems the tests run it on.  ``gmres_shifted`` is ``gmres_adjoint`` of
tests/adjoint_gmres_ref.py with the shift and the linear measure: ``shift * d = A d + b`` from ``d = 0``, residual
``r = A d + b - shift * d``, ``rel = |r| / |b|``, tolerance ``rel <= eta``, inner target ``|g_{j+1}| <= eta * |b|``, ``shift`` on
the Hessenberg's diagonal; everything else -- head-of-cycle tests, Arnoldi on the raw products, classical Gram-Schmidt twice with a
conditional second pass, Givens rotations, lowest-residual iterate kept, stagnation and budget -- statement by statement the same."""
import math

import torch

from conftest import CASES, load_case, load_weights
from oracle import psignn_oracle as orc

FIXTURES = ("hex13_dirichlet_s0", "hex13_mixed_s1")
CASE_NAMES = FIXTURES + ("two layers dirichlet", "two layers mixed")
SHIFTS = (1.0, 1.5)
B_SEED = 0   # the seed of b = randn: every case's permuted runs agree on the counts with it (scripts/calib_f64_newton.py)


def gmres_shifted(op, b, shift, eta, max_products, m=50, device=None):
    """Solve shift * d = op(d) + b from d = 0.  Returns the solver dict of ``engine.DeviceGmres64.solve_shifted``."""
    shape = b.shape
    b = b.reshape(-1)
    A = lambda v: op(v.view(shape)).reshape(-1)
    y = torch.zeros_like(b)
    nb = float(b.norm())
    products = cycles = n_reorth = 0
    prev_rel = lowest = best = None
    rel_trace, abs_trace = [], []
    while True:
        if cycles == 0:
            r = b.clone()
        else:
            r = (A(y) + b) - shift * y
            products += 1
        nr = float(r.norm())
        rel = 0.0 if nr == 0.0 else nr / nb
        rel_trace.append(rel)
        abs_trace.append(nr)
        if lowest is None or rel < lowest:
            lowest, best = rel, y.clone()
        c, cycles = cycles, cycles + 1
        left = min(m, max_products - products - 1)
        if rel <= eta or nr == 0.0:
            stop = "tolerance"
            break
        if c > 0 and not rel <= 0.5 * prev_rel:
            stop = "stagnation"
            break
        if left <= 0:
            stop = "budget"
            break
        prev_rel = rel
        V = torch.zeros((left + 1, b.numel()), dtype=b.dtype, device=device)
        V[0] = r / nr
        R = torch.zeros((left + 1, left), dtype=torch.float64)
        g = torch.zeros(left + 1, dtype=torch.float64)
        g[0] = nr
        cs, sn = [], []
        k = 0
        for j in range(left):
            w = A(V[j])
            products += 1
            n0 = float(w.double() @ w.double())
            h1 = V[:j + 1] @ w
            w = w - h1 @ V[:j + 1]
            h = h1.double().cpu()
            if not float(w.double() @ w.double()) >= 0.5 * n0:   # Daniel-Gragg-Kaufman-Stewart
                h2 = V[:j + 1] @ w
                w = w - h2 @ V[:j + 1]
                h = h + h2.double().cpu()
                n_reorth += 1
            hn = float(w.norm())
            col = torch.cat([h, torch.tensor([hn], dtype=torch.float64)])
            col[j] -= shift   # Hessenberg of A - shift I from the Arnoldi relation of A
            for i in range(j):
                t = cs[i] * col[i] + sn[i] * col[i + 1]
                col[i + 1] = -sn[i] * col[i] + cs[i] * col[i + 1]
                col[i] = t
            a, bb = float(col[j]), float(col[j + 1])
            rr = math.hypot(a, bb)
            ci, si = (a / rr, bb / rr) if rr > 0.0 else (1.0, 0.0)
            cs.append(ci)
            sn.append(si)
            col[j], col[j + 1] = rr, 0.0
            R[:j + 2, j] = col
            g[j + 1] = -si * g[j]
            g[j] = ci * g[j]
            k = j + 1
            if abs(float(g[j + 1])) <= eta * nb or k >= left or not hn > 0.0:
                break
            V[j + 1] = w / hn
        z = torch.zeros(k, dtype=torch.float64)
        for i in range(k - 1, -1, -1):
            s = g[i] - R[i, i + 1:k] @ z[i + 1:k]
            z[i] = s / R[i, i] if float(R[i, i]) != 0.0 else 0.0
        y = y - z.to(b.dtype).to(V.device) @ V[:k]   # (A - shift I) z = r: the correction that cancels r is -z
    return {"result": best.view(shape), "nstep": products, "lowest": lowest, "rel_trace": rel_trace, "abs_trace": abs_trace,
            "n_cycles": cycles, "stop": stop, "n_reorth": n_reorth}


def to64(sd, mesh):
    m64 = mesh.clone()
    for k, v in list(vars(mesh).items()):
        if torch.is_tensor(v) and v.is_floating_point():
            setattr(m64, k, v.double())
    return {k: v.double() for k, v in sd.items()}, m64


def case_inputs(name):
    """(fixture name, state dict) of one of ``CASE_NAMES``: the shipped checkpoint of a stored fixture, or a random two-layer block
    of a family on its hex13 mesh."""
    if name in FIXTURES:
        return name, load_weights(CASES[name])
    from test_gpu_f64 import _random_two_layer_mixed
    from test_gpu_plan_limits import _random_two_layer
    mixed = name.endswith("mixed")
    return ("hex13_mixed_s1" if mixed else "hex13_dirichlet_s0"), (_random_two_layer_mixed() if mixed else _random_two_layer())


class LinearProblem:
    """One linear problem on the float64 CPU oracle: the mesh of a stored fixture, a state dict, the state = the fixture's stored
    ``fp64_result``, ``b = randn`` (seed ``B_SEED``), ``w = randn`` (the next draw: the dual vector of the duality test).  ``jvp`` /
    ``vjp``: ``v -> J_f(H) v`` / ``J_f(H)^T v`` by autograd through ``orc.function_forward`` in float64 (one graph each, kept).
    ``mesh``: the fixture's mesh in another edge order (the calibration); the default is the stored one."""

    def __init__(self, name, mesh=None, seed=B_SEED):
        self.name = name
        fixture, self.sd = case_inputs(name)
        self.golden, stored = load_case(fixture)
        self.mesh = stored if mesh is None else mesh
        self.s64, self.m64 = to64(self.sd, self.mesh)
        self.H = torch.from_numpy(self.golden["fp64_result"]).double()
        with torch.no_grad():
            self.h0 = orc.encoder(self.s64, self.m64.x)
        gen = torch.Generator().manual_seed(seed)
        self.b = torch.randn(self.H.shape, generator=gen, dtype=torch.float64)
        self.w = torch.randn(self.H.shape, generator=gen, dtype=torch.float64)
        hh = self.H.clone().requires_grad_(True)
        out = orc.function_forward(self.s64, hh, self.h0, self.m64)
        u = torch.zeros_like(out, requires_grad=True)
        self._out, self._hh, self._u = out, hh, u
        self._gu = torch.autograd.grad(out, hh, u, create_graph=True)[0]   # J^T u, linear in u: its VJP with v is J v

    def vjp(self, v):
        return torch.autograd.grad(self._out, self._hh, v, retain_graph=True)[0]

    def jvp(self, v):
        return torch.autograd.grad(self._gu, self._u, v, retain_graph=True)[0]

    def op(self, transposed):
        return self.vjp if transposed else self.jvp

    def solve(self, shift, transposed, eta=1e-2, max_products=200, m=50, b=None):
        return gmres_shifted(self.op(transposed), self.b if b is None else b, shift, eta, max_products, m=m)
