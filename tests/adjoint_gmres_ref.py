"""Torch restatement of the restarted GMRES adjoint solve (csrc/krylov.hip, ``adjoint_gmres_loop``) and the CPU problems the
tests run it on.  The cycle logic is the device's, statement by statement: residual and stop tests at the head of a cycle, Arnoldi
on the raw products with classical Gram-Schmidt applied twice (second pass conditional), Givens rotations in float64 with the
shift on the Hessenberg's diagonal, ``y -= V z`` at the end.  Vectors keep the dtype of ``grad`` (float32: what the device does;
float64: the truth the tests compare against)."""
import math

import torch

from conftest import CASES, load_case, load_weights
from oracle import psignn_oracle as orc

FIXTURES = ("hex13_dirichlet_s0", "hex26_dirichlet_s0", "hex13_mixed_s1")


def gmres_adjoint(vjp, grad, eps, max_products, m=50, device=None):
    """Solve y = vjp(y) + grad from y = 0.  Returns the solver dict of ``engine.DeviceGmres.solve_adjoint``.  ``device``: where the
    basis is allocated (default: the CPU, where the stored problems live); with ``grad`` and ``vjp`` on a GPU the vector work runs
    there as plain torch, the small Hessenberg problem stays on the CPU in float64 either way."""
    shape = grad.shape
    b = grad.reshape(-1)
    op = lambda v: vjp(v.view(shape)).reshape(-1)
    y = torch.zeros_like(b)
    products = cycles = n_reorth = 0
    prev_rel = lowest = best = None
    rel_trace, abs_trace = [], []
    while True:
        if cycles == 0:
            f = b.clone()
        else:
            f = op(y) + b
            products += 1
        r = f - y
        nr, nf = float(r.norm()), float(f.norm())
        rel = nr / (nf + 1e-9)
        rel_trace.append(rel)
        abs_trace.append(nr)
        if lowest is None or rel < lowest:
            lowest, best = rel, y.clone()
        c, cycles = cycles, cycles + 1
        left = min(m, max_products - products - 1)
        if rel < eps or nr == 0.0:
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
            w = op(V[j])
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
            col[j] -= 1.0   # Hessenberg of J^T - I from the Arnoldi relation of J^T
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
            if abs(float(g[j + 1])) <= 0.5 * eps * nf or k >= left or not hn > 0.0:
                break
            V[j + 1] = w / hn
        z = torch.zeros(k, dtype=torch.float64)
        for i in range(k - 1, -1, -1):
            s = g[i] - R[i, i + 1:k] @ z[i + 1:k]
            z[i] = s / R[i, i] if float(R[i, i]) != 0.0 else 0.0
        y = y - z.to(b.dtype).to(V.device) @ V[:k]   # (J^T - I) z = r: the correction that cancels r is -z
    return {"result": best.view(shape), "nstep": products, "lowest": lowest, "rel_trace": rel_trace, "abs_trace": abs_trace,
            "n_cycles": cycles, "stop": stop, "n_reorth": n_reorth}


def stacked_dirichlet(L):
    """The trained dirichlet checkpoint with its layer 0 copied into layers 1..L-1 (the "stacked checkpoint" of
    tests/test_gpu_multilayer.py: its fixed-point solve converges without rescaling)."""
    sd = load_weights("dirichlet")
    out = dict(sd)
    for k, t in sd.items():
        for mod in ("phi_to_list", "phi_from_list", "update_list"):
            if f".f.{mod}.0." in k:
                for l in range(1, L):
                    out[k.replace(f"{mod}.0.", f"{mod}.{l}.")] = t.clone()
    return out


class AdjointProblem:
    """The adjoint system of one stored fixture on the CPU oracle: shipped checkpoint, H* from the oracle's fp32 Broyden at 1e-6,
    ``grad = randn`` with seed 0.  ``vjp32`` / ``vjp64``: w -> J_f(H*)^T w on the float32 / float64 oracle (one autograd graph
    each, kept).  ``sd``: another state dict than the fixture's shipped checkpoint."""

    def __init__(self, name, seed=0, sd=None):
        self.name = name
        self.golden, self.mesh = load_case(name)
        self.sd = load_weights(CASES[name]) if sd is None else sd
        with torch.no_grad():
            self.h0 = orc.encoder(self.sd, self.mesh.x)
            self.h_star = orc.broyden(lambda H: orc.function_forward(self.sd, H, self.h0, self.mesh), self.h0, threshold=500,
                                      eps=1e-6)["result"].clone()
        self.grad = torch.randn(self.h_star.shape, generator=torch.Generator().manual_seed(seed))
        self._g32 = self._graph(self.sd, self.mesh, self.h0, self.h_star)
        sd64 = {k: v.double() for k, v in self.sd.items()}
        m64 = self.mesh.clone()
        for k in m64.keys():
            v = getattr(m64, k)
            if torch.is_tensor(v) and v.is_floating_point():
                setattr(m64, k, v.double())
        self._g64 = self._graph(sd64, m64, self.h0.double(), self.h_star.double())
        self._truth = None

    @staticmethod
    def _graph(sd, mesh, h0, h_star):
        hh = h_star.detach().clone().requires_grad_(True)
        return orc.function_forward(sd, hh, h0, mesh), hh

    def vjp32(self, w):
        return torch.autograd.grad(self._g32[0], self._g32[1], w, retain_graph=True)[0]

    def vjp64(self, w):
        return torch.autograd.grad(self._g64[0], self._g64[1], w, retain_graph=True)[0]

    def truth(self):
        """The float64 adjoint: float64 GMRES to 1e-13 on the float64 oracle VJP."""
        if self._truth is None:
            out = gmres_adjoint(self.vjp64, self.grad.double(), 1e-13, 5000, m=100)
            assert out["lowest"] < 1e-12, out["lowest"]
            self._truth = out["result"]
        return self._truth

    def error(self, y):
        t = self.truth()
        return float((y.detach().double().cpu() - t).norm() / t.norm())

    def broyden32(self, eps=1e-8, threshold=500):
        """The oracle's fp32 Broyden on the same system: (solver dict, products)."""
        n = [0]

        def f(y):
            n[0] += 1
            return self.vjp32(y) + self.grad
        out = orc.broyden(f, torch.zeros_like(self.grad), threshold=threshold, eps=eps)
        return out, n[0]
