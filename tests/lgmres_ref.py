"""Torch restatement of the float64 GMRES with augmented restarts (LGMRES; Baker, Jessup, Manteuffel 2005) and a settable stall
ratio (csrc/krylov_f64.hip, ``psignn_gmres64_solve_adjoint_opts`` / ``psignn_gmres64_solve_shifted_opts``).  ``lgmres_adjoint`` is
``gmres_adjoint`` of tests/adjoint_gmres_ref.py (``lin=True``: ``gmres_shifted`` of tests/newton64_ref.py) plus the statements of the
method as the header of krylov_f64.hip gives them, and nothing else: the ring of corrections, the cycle plan, the augmentation step
and the stall ratio.  With ``augment=0, stall=0.5`` every operation is the one of those two functions, in their order."""
import math

import torch


def plan(stored, augment, left):
    """(nk, ka) of a cycle: Krylov steps and augmentation steps (``lgm_plan_*`` of csrc/gmres_dense.h)."""
    ka = max(0, min(stored, augment, left - 1))
    return left - ka, ka


def lgmres_adjoint(vjp, grad, eps, max_products, m=50, augment=0, stall=0.5, shift=1.0, lin=False, device=None):
    """``lin=False``: solve y = vjp(y) + grad from y = 0 with Broyden's measure, as ``gmres_adjoint`` does (``shift`` must be 1).
    ``lin=True``: solve shift * y = vjp(y) + grad from y = 0 with the linear measure |r| / |grad|, tolerance ``rel <= eps`` and inner
    target ``eps * |grad|``, as ``gmres_shifted`` does (``vjp`` is then any linear operator).  Returns their dict plus ``n_aug``."""
    assert lin or shift == 1.0
    shape = grad.shape
    b = grad.reshape(-1)
    op = lambda v: vjp(v.view(shape)).reshape(-1)
    y = torch.zeros_like(b)
    nb = float(b.norm())
    products = cycles = n_reorth = n_aug = 0
    prev_rel = lowest = best = None
    rel_trace, abs_trace = [], []
    ring = []   # the kept corrections dy / |dy|, newest first; cleared here, at the start of the solve
    while True:
        if lin:
            if cycles == 0:
                r = b.clone()
            else:
                r = (op(y) + b) - shift * y
                products += 1
            nr = float(r.norm())
            nf = nb
            rel = 0.0 if nr == 0.0 else nr / nb
        else:
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
        if (rel <= eps if lin else rel < eps) or nr == 0.0:
            stop = "tolerance"
            break
        if c > 0 and not rel <= stall * prev_rel:
            stop = "stagnation"
            break
        if left <= 0:
            stop = "budget"
            break
        prev_rel = rel
        nk, ka = plan(len(ring), augment, left)   # the cycle plan
        target = eps * nb if lin else 0.5 * eps * nf
        V = torch.zeros((left + 1, b.numel()), dtype=b.dtype, device=device)
        V[0] = r / nr
        R = torch.zeros((left + 1, left), dtype=torch.float64)
        g = torch.zeros(left + 1, dtype=torch.float64)
        g[0] = nr
        cs, sn = [], []
        k = 0
        for j in range(left):
            if j < nk:   # Krylov step
                w = op(V[j])
            else:        # augmentation step: the (j - nk)-th newest correction; the shift cannot sit on the diagonal
                zh = ring[j - nk]
                w = op(zh)
                w = w - shift * zh
                n_aug += 1
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
            if j < nk:
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
            if abs(float(g[j + 1])) <= target or k >= left or not hn > 0.0:
                break
            V[j + 1] = w / hn
        z = torch.zeros(k, dtype=torch.float64)
        for i in range(k - 1, -1, -1):
            s = g[i] - R[i, i + 1:k] @ z[i + 1:k]
            z[i] = s / R[i, i] if float(R[i, i]) != 0.0 else 0.0
        zt = z.to(b.dtype).to(V.device)
        kb = min(k, nk)
        dy = zt[:kb] @ V[:kb]   # (A - shift I) [V_kb, zhat ..] z = r: the correction that cancels r is -dy
        if k > nk:
            dy = dy + zt[nk:k] @ torch.stack(ring[:k - nk])
        y = y - dy
        if augment > 0:   # the ring: the newest first, the `augment` newest kept
            n = float(dy.norm())
            if n > 0.0 and math.isfinite(n):
                ring.insert(0, dy / n)
                del ring[augment:]
    return {"result": best.view(shape), "nstep": products, "lowest": lowest, "rel_trace": rel_trace, "abs_trace": abs_trace,
            "n_cycles": cycles, "stop": stop, "n_reorth": n_reorth, "n_aug": n_aug}
