"""Host-side handles of the HIP hot path: mesh plan, packed weights, f / JVP, device Broyden.

Everything numerical happens in libpsignn_hip.so; this module only owns lifetimes, packs the
reference ``state_dict`` into the flat weight buffer (layout: csrc/common.h ``WLayout``) and passes
device pointers.
"""
from __future__ import annotations

import ctypes as C
import math
import weakref

import numpy as np
import torch

from . import _native as nat

D = nat.D                                # the default latent width (libpsignn_hip.so: every entry point)
SUPPORTED_WIDTHS = nat.SUPPORTED_WIDTHS  # widths with a library; other than D: forward inference only (libpsignn_hip_d<w>.so)


def width_of(sd) -> int:
    """Latent width of a reference state dict (``deqdss.f.laynorm.weight``); NativeError listing the supported widths otherwise."""
    return nat.check_width(sd["deqdss.f.laynorm.weight"].numel())


# ---------------------------------------------------------------------------------------------
# weights
# ---------------------------------------------------------------------------------------------
def is_mixed_state_dict(sd) -> bool:
    return any(k.startswith("deqdss.f.phi_neumann") for k in sd)


def n_layers_of(sd) -> int:
    return 1 + max(int(k.split(".")[3]) for k in sd if k.startswith("deqdss.f.update_list."))


def pack_weights(sd, device=None) -> torch.Tensor:
    """Flatten the ``deqdss.f.*`` tensors of a reference state_dict into the kernel layout.

    Key layout of the reference: dirichlet/psignn/model.py:265-277 (mixed/psignn/model.py:198-214),
    SURVEY §8b.  Order (csrc/common.h): shared{ln_gamma, ln_beta, alpha_w, alpha_b} padded to a multiple of 16 (64 at d = 10);
    per layer phi_to{W1,b1,W2,b2} phi_from{..} update{U1,c1,U2,c2}; mixed tail phi_neumann, update_neumann.
    The latent width d is read from the state dict; every size below is WLayout's expression in d (at d = 10: 64, 244, 112,
    950, 620), and ``PackedWeights`` checks the total against the library of that width.
    """
    D = width_of(sd)   # (shadows the module's default width: the layout below is written in terms of this state dict's)
    mixed = is_mixed_state_dict(sd)
    nl = n_layers_of(sd)
    P = "deqdss.f."
    g = lambda k: sd[P + k].detach().to("cpu", torch.float32).reshape(-1)
    p = 3 if mixed else 2
    rup = lambda n, k: (n + k - 1) // k * k
    shared_sz, fold_sz, nfold_sz = rup(5 * D + 4, 16), rup(2 * D * D + 4 * D + 2, 4), rup(D * D + D, 4)
    tpl_sz, tpn_sz = 8 * D * D + 15 * D, 5 * D * D + 12 * D
    if sd[P + "alpha.0.weight"].numel() != 3 * D + p:
        raise nat.NativeError("alpha gate width does not match the boundary-condition family")
    shared = torch.cat([g("laynorm.weight"), g("laynorm.bias"), g("alpha.0.weight"), g("alpha.0.bias")])
    parts = [torch.nn.functional.pad(shared, (0, shared_sz - shared.numel()))]
    for l in range(nl):
        for phi in ("phi_to_list", "phi_from_list"):
            parts += [g(f"{phi}.{l}.mlp.mlp.0.weight"), g(f"{phi}.{l}.mlp.mlp.0.bias"),
                      g(f"{phi}.{l}.mlp.mlp.2.weight"), g(f"{phi}.{l}.mlp.mlp.2.bias")]
        parts += [g(f"update_list.{l}.mlp.0.weight"), g(f"update_list.{l}.mlp.0.bias"),
                  g(f"update_list.{l}.mlp.2.weight"), g(f"update_list.{l}.mlp.2.bias")]
        # fold block: second Phi layer pushed through the consumers of mp_to / mp_from (float64, rounded once)
        m = lambda k: sd[P + k].detach().to("cpu", torch.float64)
        U1, wa = m(f"update_list.{l}.mlp.0.weight"), m("alpha.0.weight").reshape(-1)
        fold = []
        for phi, c0 in (("phi_to_list", D), ("phi_from_list", 2 * D)):
            W2, b2 = m(f"{phi}.{l}.mlp.mlp.2.weight"), m(f"{phi}.{l}.mlp.mlp.2.bias")
            fold += [(U1[:, c0:c0 + D] @ W2).reshape(-1), U1[:, c0:c0 + D] @ b2]
        for phi, c0 in (("phi_to_list", D), ("phi_from_list", 2 * D)):
            fold.append(wa[c0:c0 + D] @ m(f"{phi}.{l}.mlp.mlp.2.weight"))
        for phi, c0 in (("phi_to_list", D), ("phi_from_list", 2 * D)):
            fold.append((wa[c0:c0 + D] @ m(f"{phi}.{l}.mlp.mlp.2.bias")).reshape(1))
        fold = torch.cat(fold).to(torch.float32)
        parts.append(torch.nn.functional.pad(fold, (0, fold_sz - fold.numel())))
    if mixed:
        parts += [g("phi_neumann.mlp.mlp.0.weight"), g("phi_neumann.mlp.mlp.0.bias"),
                  g("phi_neumann.mlp.mlp.2.weight"), g("phi_neumann.mlp.mlp.2.bias"),
                  g("update_neumann.mlp.0.weight"), g("update_neumann.mlp.0.bias"),
                  g("update_neumann.mlp.2.weight"), g("update_neumann.mlp.2.bias")]
        m = lambda k: sd[P + k].detach().to("cpu", torch.float64)
        N1 = m("update_neumann.mlp.0.weight")
        nf = torch.cat([(N1[:, D:2 * D] @ m("phi_neumann.mlp.mlp.2.weight")).reshape(-1),
                        N1[:, D:2 * D] @ m("phi_neumann.mlp.mlp.2.bias")]).to(torch.float32)
        parts.append(torch.nn.functional.pad(nf, (0, nfold_sz - nf.numel())))
    # ---- transposed section for the tile kernel: [in k][out o] blocks (WLayout::T_* / N_*)
    m = lambda k: sd[P + k].detach().to("cpu", torch.float64)
    f32 = lambda t: t.to(torch.float32).reshape(-1)

    def padto(t, n):
        t = f32(t)
        return torch.nn.functional.pad(t, (0, n - t.numel()))
    mir = torch.tensor([-1.0, -1.0, 1.0], dtype=torch.float64)[:, None]  # in-edge attr = mirror of the stored out-edge attr
    for l in range(nl):
        Wt, Wf = m(f"phi_to_list.{l}.mlp.mlp.0.weight"), m(f"phi_from_list.{l}.mlp.mlp.0.weight")
        U1, U2 = m(f"update_list.{l}.mlp.0.weight"), m(f"update_list.{l}.mlp.2.weight")
        G_to = U1[:, D:2 * D] @ m(f"phi_to_list.{l}.mlp.mlp.2.weight")
        G_fr = U1[:, 2 * D:3 * D] @ m(f"phi_from_list.{l}.mlp.mlp.2.weight")
        g_to = U1[:, D:2 * D] @ m(f"phi_to_list.{l}.mlp.mlp.2.bias")
        g_fr = U1[:, 2 * D:3 * D] @ m(f"phi_from_list.{l}.mlp.mlp.2.bias")
        tp = [f32(Wt[:, D:2 * D].t()), f32(Wf[:, D:2 * D].t()), f32(Wt[:, :D].t()), f32(Wf[:, :D].t()),
              f32(Wt[:, 2 * D:].t() * mir), f32(Wf[:, 2 * D:].t()),
              f32(m(f"phi_to_list.{l}.mlp.mlp.0.bias")), f32(m(f"phi_from_list.{l}.mlp.mlp.0.bias")),
              f32(U1[:, :D].t()), f32(G_to.t()), f32(G_fr.t()), padto(U1[:, 3 * D:].t(), 3 * D),
              f32(m(f"update_list.{l}.mlp.0.bias")), f32(g_to), f32(g_fr), f32(U2.t()),
              f32(m(f"update_list.{l}.mlp.2.bias"))]
        tp = torch.cat(tp)
        assert tp.numel() == tpl_sz
        parts.append(tp)
    if mixed:
        Wn, N1, N2 = m("phi_neumann.mlp.mlp.0.weight"), m("update_neumann.mlp.0.weight"), m("update_neumann.mlp.2.weight")
        Gn = N1[:, D:2 * D] @ m("phi_neumann.mlp.mlp.2.weight")
        gn = N1[:, D:2 * D] @ m("phi_neumann.mlp.mlp.2.bias")
        tn = torch.cat([f32(Wn[:, D:2 * D].t()), f32(Wn[:, :D].t()), f32(Wn[:, 2 * D:].t()),
                        f32(m("phi_neumann.mlp.mlp.0.bias")), f32(N1[:, :D].t()), f32(Gn.t()),
                        padto(N1[:, 2 * D:].t(), 5 * D), f32(m("update_neumann.mlp.0.bias")), f32(gn), f32(N2.t()),
                        f32(m("update_neumann.mlp.2.bias"))])
        assert tn.numel() == tpn_sz
        parts.append(tn)
    flat = torch.cat(parts).contiguous()
    return flat if device is None else flat.to(device)


class PackedWeights:
    def __init__(self, sd, device):
        self.mixed = is_mixed_state_dict(sd)
        self.n_layers = n_layers_of(sd)
        self.width = width_of(sd)
        self.lib = nat.lib(self.width)   # the library these weights are packed for; the maps made from them call it
        self.flat = pack_weights(sd, device)
        expect = self.lib.psignn_weights_size(int(self.mixed), self.n_layers)
        if self.flat.numel() != expect:
            raise nat.NativeError(f"packed weight length {self.flat.numel()} != native layout {expect} at latent_dim {self.width}")


# ---------------------------------------------------------------------------------------------
# mesh plan
# ---------------------------------------------------------------------------------------------
_EXPORT = {"csr_ptr": (0, np.int32), "csr_nbr": (1, np.int32), "csr_eid": (2, np.int32),
           "csc_ptr": (3, np.int32), "csc_nbr": (4, np.int32), "csc_eid": (5, np.int32),
           "node_flags": (6, np.uint8), "csr_attr": (7, np.float32), "csc_attr": (8, np.float32),
           "a_ptr": (9, np.int32), "a_col": (10, np.int32), "a_val": (11, np.float32),
           "perm": (12, np.int32), "tile_ptr": (13, np.int32), "halo_cnt": (14, np.int32), "halo": (15, np.int32),
           "slice_off": (16, np.int32), "slice_deg": (17, np.uint8), "ell": (18, np.uint32),
           "tile_slice": (20, np.int32)}

HALO_CAP = 512


class MeshPlan:
    """Iteration-invariant device data of one mesh (or a disjoint union).  See csrc/plan.hip."""

    def __init__(self, batch, tile_target=0):
        """tile_target: nodes per tile (0 = library default, < 0 = untiled global-gather kernels)."""
        ei = batch.edge_index
        nat.require_cuda(ei, "batch.edge_index")
        self.device = ei.device
        N = int(batch.x.shape[0])
        tags = batch.tags.to(torch.float32).contiguous()
        if tags.dim() == 1:
            tags = tags[:, None]
        ea = batch.edge_attr.to(torch.float32).contiguous()
        aij = getattr(batch, "a_ij", None)
        aij = None if aij is None else aij.to(torch.float32).reshape(-1).contiguous()
        eic = ei.to(torch.int64).contiguous()
        if ea.shape[0] != eic.shape[1] or ea.shape[1] != 3:
            raise nat.NativeError(f"edge_attr shape {tuple(ea.shape)} does not match edge_index {tuple(eic.shape)}")
        if tags.shape[0] != N:
            raise nat.NativeError("tags and x disagree on the node count")
        pos = getattr(batch, "pos", None)
        if pos is not None:
            pos = pos.to(torch.float32).contiguous()
            if pos.shape != (N, 2) or pos.device != self.device:
                pos = None  # coordinates only steer the tiling; without them the given numbering is kept
        gid = getattr(batch, "batch", None)
        if pos is not None and gid is not None and gid.numel() == N and int(gid.max()) > 0:
            # disjoint union of graphs (PyG Batch): the graphs overlap in space, which would mix them inside a tile.
            # Shift graph g by g bounding-box widths for the TILING only (positions never enter the arithmetic).
            span = (pos[:, 0].max() - pos[:, 0].min()) * 1.05 + 1e-6
            pos = pos.clone()
            pos[:, 0] += gid.to(pos.dtype) * span
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            nat.check(nat.lib().psignn_plan_create(C.byref(h), N, eic.shape[1], nat.ptr(eic), nat.ptr(ea),
                                                   nat.ptr(aij), nat.ptr(tags), tags.shape[1], nat.ptr(pos),
                                                   int(tile_target), nat.stream_ptr(self.device)),
                      "psignn_plan_create")
        self.handle = h
        self._fin = weakref.finalize(self, nat.lib().psignn_plan_destroy, h)
        self.N = N
        self.E = int(eic.shape[1])
        self.Ep = int(nat.lib().psignn_plan_num_nonself_edges(h))
        self.mixed = tags.shape[1] == 3
        self.tiled = bool(nat.lib().psignn_plan_is_tiled(h))
        self.n_tiles = int(nat.lib().psignn_plan_num_tiles(h))
        self.ell_rows = int(nat.lib().psignn_plan_ell_rows(h))
        self.max_tile_rows = int(nat.lib().psignn_plan_max_tile_rows(h))
        self._work = None
        self._pwork = None
        self._jwork = None

    def export(self, name):
        which, dt = _EXPORT[name]
        if which >= 12 and not self.tiled:
            raise nat.NativeError("plan has no tile structures")
        n_slices = None
        if name in ("slice_off", "slice_deg"):
            n_slices = int(self.export("tile_slice")[-1])
        n = {"csr_ptr": self.N + 1, "csc_ptr": self.N + 1, "a_ptr": self.N + 1, "node_flags": self.N,
             "csr_attr": 3 * self.Ep, "csc_attr": 3 * self.Ep, "a_col": self.E, "a_val": self.E,
             "perm": self.N, "tile_ptr": self.n_tiles + 1, "tile_slice": self.n_tiles + 1, "halo_cnt": self.n_tiles,
             "halo": self.n_tiles * HALO_CAP, "slice_off": (n_slices or 0) + 1, "slice_deg": (n_slices or 0),
             "ell": self.ell_rows * 64 * 4}.get(name, self.Ep)
        out = np.empty(n, dtype=dt)
        nat.check(nat.lib().psignn_plan_export(self.handle, which, out.ctypes.data_as(C.c_void_p), out.nbytes),
                  "psignn_plan_export")
        return out

    def _grown(self, attr, query, n_layers, lib=None):
        """One scratch buffer per kind, grown in place of the old one when more is needed: ``lib``'s own count for the kind
        (``query``: the name of its ``*_workspace_floats`` entry) plus, at the default width, the layer workspace of a
        multi-layer block (``psignn_f_layers_workspace_floats``; the width libraries hold no derivative of a layer chain)."""
        lib = lib or nat.lib()
        n = int(getattr(lib, query)(self.handle))
        if lib.width == D:
            extra = int(lib.psignn_f_layers_workspace_floats(self.handle, int(n_layers)))
            if extra < 0:
                raise nat.NativeError(f"n_layers = {n_layers} is out of range")
            n += extra
        buf = getattr(self, attr)
        if buf is None or buf.numel() < n:
            buf = torch.empty(n, dtype=torch.float32, device=self.device)
            setattr(self, attr, buf)
        return buf

    def workspace(self, lib=None):
        """Scratch of f.  The plan itself is width-free (one plan serves maps of every latent width); the scratch is sized by
        the library that is about to use it (``lib``: a ``nat.lib(width)``, default the default width's) and only ever grows."""
        return self._grown("_work", "psignn_f_workspace_floats", 1, lib)

    def derivative_workspace(self, n_layers):
        """Scratch of the JVP / VJP entry points: ``workspace()``'s buffer, grown for a multi-layer block's layer states."""
        return self._grown("_work", "psignn_f_workspace_floats", n_layers)

    def pgrad_workspace(self, n_layers=1):
        return self._grown("_pwork", "psignn_f_param_vjp_workspace_floats", n_layers)

    def vjp_backward_workspace(self, n_layers=1):
        return self._grown("_jwork", "psignn_f_vjp_backward_workspace_floats", n_layers)

    def vjp_backward_p_workspace(self):
        """Scratch of the plan-order (tile) backward of the VJP; shares ``vjp_backward_workspace()``'s buffer."""
        return self._grown("_jwork", "psignn_f_vjp_backward_p_workspace_floats", 1)

    def permute(self, t, to_plan=True):
        """Rows of an (N, cols) float tensor between the caller's numbering and plan order."""
        tc = _f32c(t)
        out = torch.empty_like(tc)
        with torch.cuda.device(self.device):
            nat.check(nat.lib().psignn_plan_permute(self.handle, nat.ptr(tc), tc.shape[1], nat.ptr(out), int(to_plan),
                                                    nat.stream_ptr(self.device)), "psignn_plan_permute")
        return out


def plan_for(batch, tile_target=0) -> MeshPlan:
    """Plan cached on the batch object (rebuilt if edge_index/tags storage changed)."""
    key = (batch.edge_index.data_ptr(), tuple(batch.edge_index.shape), batch.tags.data_ptr(),
           batch.edge_attr.data_ptr(), str(batch.edge_index.device), tile_target)
    cached = getattr(batch, "_psignn_plan", None)
    if cached is not None and cached[0] == key:
        return cached[1]
    plan = MeshPlan(batch, tile_target)
    try:
        batch._psignn_plan = (key, plan)
    except Exception:
        pass
    return plan


def _f32c(t):
    return t.to(torch.float32).contiguous()


class FixedPointMap:
    """``H -> f(H, H_init, batch)`` bound to a plan and packed weights.

    Stands where the reference passes ``lambda H: self.f(H, H_init, batch)`` to the solver
    (dirichlet/psignn/model.py:189, tests/model_psignn.py:226).  Being an object instead of a lambda lets
    ``utilities.solver.broyden`` recognise it and run the whole root-find on the device.
    """

    def __init__(self, plan: MeshPlan, weights: PackedWeights, h_initial, prb_data, normals=None):
        if plan.mixed != weights.mixed:
            raise nat.NativeError("boundary-condition family of the weights and of the batch differ "
                                  f"(weights mixed={weights.mixed}, batch mixed={plan.mixed})")
        self.plan, self.weights = plan, weights
        self.width, self.lib = weights.width, weights.lib
        self.h0 = _f32c(h_initial)
        self.prb = _f32c(prb_data)
        self.nrm = None if normals is None else _f32c(normals)
        if plan.mixed and self.nrm is None:
            raise nat.NativeError("mixed problems need batch.unit_normal_vector")
        exp_p = 3 if plan.mixed else 2
        if self.prb.shape != (plan.N, exp_p) or self.h0.shape != (plan.N, self.width):
            raise nat.NativeError(f"shape mismatch: prb_data {tuple(self.prb.shape)}, h_initial {tuple(self.h0.shape)} "
                                  f"(weights of latent_dim {self.width})")
        self._p = None  # plan-order copies of h0 / prb / normals, made on first use

    lin_neumann = "direct"   # what ``linearize_p`` gives a new Linearization (the model sets its ``lin_neumann`` config value)
    jac_backward = "gather"  # the route the Jacobian regulariser's backward takes (the model sets its ``jac_backward`` config value)

    # -- plan-order fast path (no permutation passes per call) -------------------------------------
    def to_plan(self, H):
        return self.plan.permute(H, True)

    def from_plan(self, Hp):
        return self.plan.permute(Hp, False)

    def _forward_only(self, what):
        nat.require_default_width(self.width, what)

    def _state(self, H, name="H"):
        Hc = _f32c(H)
        if Hc.shape != (self.plan.N, self.width):
            raise nat.NativeError(f"{name} has shape {tuple(Hc.shape)}, expected {(self.plan.N, self.width)}")
        return Hc

    def fp(self, Hp):
        """f in plan order: Hp and the result are numbered like the plan's tiles (see MeshPlan.permute)."""
        if self._p is None:
            self._p = (self.to_plan(self.h0), self.to_plan(self.prb), None if self.nrm is None else self.to_plan(self.nrm))
        h0p, prbp, nrmp = self._p
        Hc = self._state(Hp, "Hp")
        out = torch.empty_like(Hc)
        with torch.cuda.device(Hc.device):
            nat.check(self.lib.psignn_f_forward_p(self.plan.handle, nat.ptr(self.weights.flat), self.weights.n_layers,
                                                  nat.ptr(Hc), nat.ptr(h0p), nat.ptr(prbp), nat.ptr(nrmp),
                                                  nat.ptr(out), nat.ptr(self.plan.workspace(self.lib)),
                                                  nat.stream_ptr(Hc.device)), "psignn_f_forward_p", self.lib)
        return out

    def __call__(self, H):
        nat.require_cuda(H, "H")
        Hc = self._state(H)
        out = torch.empty_like(Hc)
        with torch.cuda.device(Hc.device):
            nat.check(self.lib.psignn_f_forward(self.plan.handle, nat.ptr(self.weights.flat), self.weights.n_layers,
                                                nat.ptr(Hc), nat.ptr(self.h0), nat.ptr(self.prb), nat.ptr(self.nrm),
                                                nat.ptr(out), nat.ptr(self.plan.workspace(self.lib)),
                                                nat.stream_ptr(Hc.device)), "psignn_f_forward", self.lib)
        return out

    def picard_p(self, Hp, n):
        """n applications of f in plan order, back to back on the device (no host work in between)."""
        if self._p is None:
            self.fp(Hp)
        h0p, prbp, nrmp = self._p
        x = self._state(Hp, "Hp").clone()
        tmp = torch.empty_like(x)
        with torch.cuda.device(x.device):
            nat.check(self.lib.psignn_picard_p(self.plan.handle, nat.ptr(self.weights.flat), self.weights.n_layers,
                                               nat.ptr(x), nat.ptr(tmp), nat.ptr(h0p), nat.ptr(prbp), nat.ptr(nrmp),
                                               nat.ptr(self.plan.workspace(self.lib)), int(n), nat.stream_ptr(x.device)),
                      "psignn_picard_p", self.lib)
        return x

    def jvp(self, H, V):
        """Analytic J_f(H) V."""
        self._forward_only("jvp")
        Hc, Vc = _f32c(H), _f32c(V)
        out = torch.empty_like(Hc)
        with torch.cuda.device(Hc.device):
            nat.check(nat.lib().psignn_f_jvp(self.plan.handle, nat.ptr(self.weights.flat), self.weights.n_layers,
                                             nat.ptr(Hc), nat.ptr(self.prb), nat.ptr(self.nrm), nat.ptr(Vc),
                                             nat.ptr(out), nat.ptr(self.plan.derivative_workspace(self.weights.n_layers)),
                                             nat.stream_ptr(Hc.device)), "psignn_f_jvp")
        return out

    def jvp_p(self, Hp, Vp, out=None):
        """J_f(Hp) Vp with everything in plan order (tiled plans, any depth; a multi-layer dirichlet block evaluates its layer
        states first).  ``out``: a contiguous (N, d) float32 tensor to write into (e.g. a row of a Krylov basis)."""
        self._forward_only("jvp_p")
        if self._p is None:
            self.fp(Hp)
        _, prbp, nrmp = self._p
        Hc, Vc = _f32c(Hp), _f32c(Vp)
        if out is None:
            out = torch.empty_like(Hc)
        elif out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != Hc.numel():
            raise nat.NativeError("jvp_p: out must be a contiguous float32 tensor of the state's size")
        with torch.cuda.device(Hc.device):
            if self.weights.mixed or self.weights.n_layers == 1:
                nat.check(nat.lib().psignn_f_jvp_p(self.plan.handle, nat.ptr(self.weights.flat), self.weights.n_layers,
                                                   nat.ptr(Hc), nat.ptr(prbp), nat.ptr(nrmp), nat.ptr(Vc), nat.ptr(out),
                                                   nat.stream_ptr(Hc.device)), "psignn_f_jvp_p")
            else:
                nat.check(nat.lib().psignn_f_jvp_pw(self.plan.handle, nat.ptr(self.weights.flat), self.weights.n_layers,
                                                    nat.ptr(Hc), nat.ptr(prbp), nat.ptr(nrmp), nat.ptr(Vc), nat.ptr(out),
                                                    nat.ptr(self.plan.derivative_workspace(self.weights.n_layers)),
                                                    nat.stream_ptr(Hc.device)), "psignn_f_jvp_pw")
        return out

    # ---- one idle Broyden solver kept between solves of this map (utilities.solver.broyden without keep_trace / solver_obj):
    # creating and destroying the 2 * threshold state vectors costs 2.2 ms per call at 1M nodes and threshold 20 -- a quarter of
    # such a solve (profiles/r3_cold_solve_probe.txt).  Bounded by PSIGNN_SOLVER_CACHE_GB (default 16; 0 disables).
    # The idle solver is keyed on (threshold, history dtype): a bf16-history call never gets an fp32 solver, nor the reverse.
    def borrow_broyden(self, threshold, history_dtype=torch.float32):
        sv = getattr(self, "_idle_broyden", None)
        self._idle_broyden = None
        if (sv is not None and sv.threshold == int(threshold) and not sv.keep_trace
                and getattr(sv, "history_dtype", torch.float32) == history_dtype):
            return sv
        if sv is not None:
            sv.close()
        return DeviceBroyden(plan=self.plan, threshold=threshold, keep_trace=False, history_dtype=history_dtype, width=self.width)

    def return_broyden(self, sv):
        import os
        limit = float(os.environ.get("PSIGNN_SOLVER_CACHE_GB", "16")) * 1e9
        old = getattr(self, "_idle_broyden", None)
        if old is not None and old is not sv:
            old.close()
        if sv.nbytes <= limit:
            self._idle_broyden = sv
        else:
            self._idle_broyden = None
            sv.close()

    def can_linearize(self):
        """True when ``linearize_p`` applies: tiled plan; dirichlet family: single-layer block (csrc/fgnn_tile_lin.hip)."""
        return self.width == D and bool(self.plan.tiled) and (bool(self.plan.mixed) or self.weights.n_layers == 1)

    def linearize_p(self, Hp, lin=None, neumann=None):
        """Linearisation of f at ``Hp`` (plan order) for solvers that apply J_f(Hp) to many vectors: one pass stores the relu
        masks and per-node gate / update / LayerNorm quantities, ``lin.jvp_p(Vp)`` then applies the Jacobian as a linear
        operator (about half the cost of ``jvp_p``, same product up to fp32 summation order).  ``lin``: a Linearization of this
        map to rebuild at the new state (keeps its device buffers).  ``neumann`` (a new handle only): ``"direct"`` or
        ``"stored"`` as in ``Linearization``; None -> the map's ``lin_neumann`` (``"direct"`` unless set)."""
        neumann = check_lin_neumann(self.lin_neumann if neumann is None else neumann)
        self._forward_only("linearize_p")
        if self._p is None:
            self.fp(Hp)
        if lin is None:
            lin = Linearization(self, neumann=neumann)
        lin.build(Hp)
        return lin

    def vjp(self, H, Wv):
        """Wv^T J_f(H): what ``autograd.grad(f(H), H, Wv)`` returns in the reference (model.py:214,432,449)."""
        self._forward_only("vjp")
        Hc, Wc = _f32c(H), _f32c(Wv)
        out = torch.empty_like(Hc)
        with torch.cuda.device(Hc.device):
            nat.check(nat.lib().psignn_f_vjp(self.plan.handle, nat.ptr(self.weights.flat), self.weights.n_layers,
                                             nat.ptr(Hc), nat.ptr(self.prb), nat.ptr(self.nrm), nat.ptr(Wc), nat.ptr(out),
                                             nat.ptr(self.plan.derivative_workspace(self.weights.n_layers)),
                                             nat.stream_ptr(Hc.device)),
                      "psignn_f_vjp")
        return out

    def vjp_p(self, Hp, Wp):
        """vjp with Hp, Wp and the result in plan order (tiled kernels where the plan has tiles, any depth)."""
        self._forward_only("vjp_p")
        if self._p is None:
            self.fp(Hp)
        _, prbp, nrmp = self._p
        Hc, Wc = _f32c(Hp), _f32c(Wp)
        out = torch.empty_like(Hc)
        with torch.cuda.device(Hc.device):
            nat.check(nat.lib().psignn_f_vjp_p(self.plan.handle, nat.ptr(self.weights.flat), self.weights.n_layers,
                                               nat.ptr(Hc), nat.ptr(prbp), nat.ptr(nrmp), nat.ptr(Wc), nat.ptr(out),
                                               nat.ptr(self.plan.derivative_workspace(self.weights.n_layers)),
                                               nat.stream_ptr(Hc.device)),
                      "psignn_f_vjp_p")
        return out

    def param_vjp_p(self, Hp, Wp):
        """(flat parameter gradient, Wp^T df/dh) at Hp, everything in plan order (tiled dirichlet plans, any depth).

        The flat gradient follows the leading section of the packed weights; ``unpack_param_grads`` names it."""
        self._forward_only("param_vjp_p")
        if self._p is None:
            self.fp(Hp)
        _, prbp, _ = self._p
        Hc, Wc = _f32c(Hp), _f32c(Wp)
        l = nat.lib()
        grad = torch.empty(int(l.psignn_param_grad_size(int(self.weights.mixed), self.weights.n_layers)),
                           dtype=torch.float32, device=Hc.device)
        out = torch.empty_like(Hc)
        work = self.plan.pgrad_workspace(self.weights.n_layers)
        with torch.cuda.device(Hc.device):
            nat.check(l.psignn_f_param_vjp_p(self.plan.handle, nat.ptr(self.weights.flat), self.weights.n_layers,
                                             nat.ptr(Hc), nat.ptr(prbp), nat.ptr(Wc), nat.ptr(grad), nat.ptr(out),
                                             nat.ptr(work), nat.stream_ptr(Hc.device)), "psignn_f_param_vjp_p")
        return grad, out

    def param_vjp(self, H, Wv):
        """What ``loss.backward()`` leaves in the ``deqdss.f`` parameters for new_H = f(H) with cotangent Wv
        (dirichlet/psignn/model.py:203-225; mixed/psignn/model.py likewise): ({name: grad}, Wv^T df/dH) in the
        caller's numbering.  Both families, any depth, tiled or not."""
        self._forward_only("param_vjp")
        grads, out, _ = self.param_vjp_init(H, Wv, with_init=False)
        return grads, out

    def param_vjp_init(self, H, Wv, with_init=True):
        """``param_vjp`` and the gradient w.r.t. h_initial: ({name: grad}, Wv^T df/dH, Wv^T df/dH_init).  The latter is the
        Dirichlet rows of the cotangent on every layer's output (those rows are copies of h_initial after every layer,
        model.py:298); for a single-layer block, Wv on the Dirichlet rows."""
        self._forward_only("param_vjp_init")
        Hc, Wc = _f32c(H), _f32c(Wv)
        l = nat.lib()
        grad = torch.empty(int(l.psignn_param_grad_size(int(self.weights.mixed), self.weights.n_layers)),
                           dtype=torch.float32, device=Hc.device)
        out = torch.empty_like(Hc)
        g_init = torch.empty_like(Hc) if with_init else None
        with torch.cuda.device(Hc.device):
            nat.check(l.psignn_f_param_vjp_ex(self.plan.handle, nat.ptr(self.weights.flat), self.weights.n_layers,
                                              nat.ptr(Hc), nat.ptr(self.prb), nat.ptr(self.nrm), nat.ptr(Wc), nat.ptr(grad),
                                              nat.ptr(out), nat.ptr(g_init),
                                              nat.ptr(self.plan.pgrad_workspace(self.weights.n_layers)),
                                              nat.stream_ptr(Hc.device)), "psignn_f_param_vjp_ex")
        return unpack_param_grads(grad, self.weights.n_layers, self.weights.mixed), out, g_init

    def can_tile_vjp_backward(self):
        """True when ``vjp_backward_p`` applies: tiled plan of the dirichlet family, single-layer block (csrc/fgnn_tile_jr.hip)."""
        return self.width == D and bool(nat.lib().psignn_f_vjp_backward_tiled_ok(self.plan.handle, int(self.weights.n_layers)))

    def vjp_backward_p(self, Hp, Vp, Gp):
        """``vjp_backward`` on the tile kernels with Hp, Vp, Gp and the returned d / dH in plan order:
        (flat parameter gradient, d / dH).  ``unpack_param_grads`` names the flat gradient.  Where
        ``can_tile_vjp_backward()`` is false this raises ``NativeError`` and launches nothing."""
        self._forward_only("vjp_backward_p")
        if not self.can_tile_vjp_backward():
            raise nat.NativeError("vjp_backward_p: the tile form needs a tiled plan of the dirichlet family and a single-layer "
                                  "block (vjp_backward takes every plan)")
        if self._p is None:
            self.fp(Hp)
        _, prbp, _ = self._p
        Hc, Vc, Gc = _f32c(Hp), _f32c(Vp), _f32c(Gp)
        l = nat.lib()
        grad = torch.empty(int(l.psignn_param_grad_size(0, self.weights.n_layers)), dtype=torch.float32, device=Hc.device)
        out = torch.empty_like(Hc)
        with torch.cuda.device(Hc.device):
            nat.check(l.psignn_f_vjp_backward_p(self.plan.handle, nat.ptr(self.weights.flat), self.weights.n_layers,
                                                nat.ptr(Hc), nat.ptr(prbp), nat.ptr(Vc), nat.ptr(Gc), nat.ptr(grad), nat.ptr(out),
                                                nat.ptr(self.plan.vjp_backward_p_workspace()), nat.stream_ptr(Hc.device)),
                      "psignn_f_vjp_backward_p")
        return grad, out

    def vjp_backward(self, H, V, Gbar, tiled=False):
        """Gradient of  Gbar . (J_f(H)^T V)  with Gbar held constant: ({name: grad}, d / dH) -- what autograd's double
        backward computes for ``autograd.grad(f(H), H, V, create_graph=True)`` (jac_loss_estimate,
        dirichlet/psignn/model.py:416-435).  Both families, any depth, caller's numbering.  ``tiled=True``: the tile
        kernels (permute in, ``vjp_backward_p``, permute out); ``NativeError`` where ``can_tile_vjp_backward()`` is false."""
        self._forward_only("vjp_backward")
        if tiled:
            flat, out_p = self.vjp_backward_p(self.to_plan(H), self.to_plan(V), self.to_plan(Gbar))
            return unpack_param_grads(flat, self.weights.n_layers, self.weights.mixed), self.from_plan(out_p)
        Hc, Vc, Gc = _f32c(H), _f32c(V), _f32c(Gbar)
        l = nat.lib()
        grad = torch.empty(int(l.psignn_param_grad_size(int(self.weights.mixed), self.weights.n_layers)),
                           dtype=torch.float32, device=Hc.device)
        out = torch.empty_like(Hc)
        with torch.cuda.device(Hc.device):
            nat.check(l.psignn_f_vjp_backward(self.plan.handle, nat.ptr(self.weights.flat), self.weights.n_layers,
                                              nat.ptr(Hc), nat.ptr(self.prb), nat.ptr(self.nrm), nat.ptr(Vc), nat.ptr(Gc), nat.ptr(grad),
                                              nat.ptr(out), nat.ptr(self.plan.vjp_backward_workspace(self.weights.n_layers)),
                                              nat.stream_ptr(Hc.device)), "psignn_f_vjp_backward")
        return unpack_param_grads(grad, self.weights.n_layers, self.weights.mixed), out

    def phi(self, H, which: int, layer: int = 0):
        """One aggregation: 0 Phi_to, 1 Phi_from, 2 Phi_neumann."""
        Hc = _f32c(H)
        out = torch.empty_like(Hc)
        with torch.cuda.device(Hc.device):
            nat.check(self.lib.psignn_phi(self.plan.handle, nat.ptr(self.weights.flat), self.weights.n_layers,
                                           layer, which, nat.ptr(Hc), nat.ptr(out), nat.ptr(self.plan.workspace(self.lib)),
                                           nat.stream_ptr(Hc.device)), "psignn_phi", self.lib)
        return out


def pack_dsgps(sd, device=None) -> torch.Tensor:
    """Flat weight buffer of the DS-GPS kernels from a ``ModelDSGPS`` state_dict (dirichlet/dsgps/model.py:35-45,
    mixed/dsgps/model.py:35-48; layout in csrc/dsgps_tile.hip): every matrix transposed to [in k][out o]."""
    m = lambda k: sd[k].detach().to("cpu", torch.float32)
    mixed = "phi_neumann.mlp.mlp.0.weight" in sd
    p = 3 if mixed else 2
    if m("phi_to.mlp.mlp.0.weight").shape != (D, 2 * D + 3) or m("z_k.mlp.0.weight").shape != (D, 3 * D + p):
        raise nat.NativeError("DS-GPS kernels are built for latent_dim = 10, 3 edge features, 2 (mixed: 3) problem features")
    t = lambda a: a.t().contiguous().reshape(-1)
    Wt, Wf = m("phi_to.mlp.mlp.0.weight"), m("phi_from.mlp.mlp.0.weight")
    mir = torch.tensor([-1.0, -1.0, 1.0])[:, None]
    parts = [t(Wt[:, D:2 * D]), t(Wf[:, D:2 * D]), t(Wt[:, :D]), t(Wf[:, :D]),
             (Wt[:, 2 * D:].t() * mir).reshape(-1), t(Wf[:, 2 * D:]),
             m("phi_to.mlp.mlp.0.bias"), m("phi_from.mlp.mlp.0.bias"),
             t(m("phi_to.mlp.mlp.2.weight")), m("phi_to.mlp.mlp.2.bias"),
             t(m("phi_from.mlp.mlp.2.weight")), m("phi_from.mlp.mlp.2.bias")]
    for g in ("z_k", "r_k", "correction"):
        parts += [t(m(f"{g}.mlp.0.weight")), m(f"{g}.mlp.0.bias")]
    if mixed:   # transposed Neumann block, same layout as the mixed PSI-GNN kernels (WLayout<3>::N_*)
        d64 = lambda k: sd[k].detach().to("cpu", torch.float64)
        f32 = lambda a: a.to(torch.float32).reshape(-1)
        Wn, N1, N2 = d64("phi_neumann.mlp.mlp.0.weight"), d64("update_neumann.mlp.0.weight"), d64("update_neumann.mlp.2.weight")
        Gn = N1[:, D:2 * D] @ d64("phi_neumann.mlp.mlp.2.weight")
        gn = N1[:, D:2 * D] @ d64("phi_neumann.mlp.mlp.2.bias")
        n1p = f32(N1[:, 2 * D:].t())
        parts += [f32(Wn[:, D:2 * D].t()), f32(Wn[:, :D].t()), f32(Wn[:, 2 * D:].t()), f32(d64("phi_neumann.mlp.mlp.0.bias")),
                  f32(N1[:, :D].t()), f32(Gn.t()), torch.nn.functional.pad(n1p, (0, 50 - n1p.numel())),
                  f32(d64("update_neumann.mlp.0.bias")), f32(gn), f32(N2.t()), f32(d64("update_neumann.mlp.2.bias"))]
    flat = torch.cat([q.reshape(-1) for q in parts]).contiguous()
    if flat.numel() != int(nat.lib().psignn_dsgps_weights_size(int(mixed))):
        raise nat.NativeError(f"packed DS-GPS weight length {flat.numel()} != native layout")
    return flat if device is None else flat.to(device)


def dsgps_forward(plan: "MeshPlan", wflat, h0, prb, k: int, nrm=None):
    """H_k of ``ModelDSGPS.inference`` (model.py:141-155): k recurrent updates from the encoder state h0."""
    nat.require_cuda(h0, "h0")
    hc, pc = _f32c(h0), _f32c(prb)
    out = torch.empty_like(hc)
    work = torch.empty(4 * plan.N * D, dtype=torch.float32, device=hc.device)
    with torch.cuda.device(hc.device):
        nat.check(nat.lib().psignn_dsgps_forward(plan.handle, nat.ptr(wflat), int(k), nat.ptr(hc), nat.ptr(pc),
                                                 nat.ptr(None if nrm is None else _f32c(nrm)), nat.ptr(out),
                                                 nat.ptr(work), nat.stream_ptr(hc.device)), "psignn_dsgps_forward")
    return out


def dsgps_step_p(plan: "MeshPlan", wflat, hp, h0p, prbp, nrmp=None):
    """One DS-GPS update, node tensors in plan order."""
    out = torch.empty_like(hp)
    with torch.cuda.device(hp.device):
        nat.check(nat.lib().psignn_dsgps_step_p(plan.handle, nat.ptr(wflat), nat.ptr(_f32c(hp)), nat.ptr(h0p), nat.ptr(prbp),
                                                nat.ptr(nrmp), nat.ptr(out), nat.stream_ptr(hp.device)), "psignn_dsgps_step_p")
    return out


# f_theta layouts (csrc/common.h WLayout<P>): shared 64 | layer 0 = phi_to 350 | phi_from 350 | update 10 (30+P) + 120 | fold 244
# [| phi_neumann 350 | update_neumann 370 | nfold 112]
_FL_PHI_TO, _FL_PHI_FROM = 64, 414
_FL_MIXED_PHI_NEU, _FL_MIXED_UPD_NEU = 64 + 700 + 450 + 244, 64 + 700 + 450 + 244 + 350


def pack_dsgps_train(sd, device):
    """(Phi modules -- mixed: and update_neumann -- in the f_theta weight layout, gates [Wz|bz|Wr|br|Wc|bc]) for
    ``psignn_dsgps_step_backward``.  Assembled on the device (no host round trip: this runs once per training forward); only
    the blocks the backward kernels read are filled."""
    mixed = "phi_neumann.mlp.mlp.0.weight" in sd
    g = lambda k: sd[k].detach().to(device, torch.float32).reshape(-1)
    n = int(nat.lib().psignn_weights_size(int(mixed), 1))
    if mixed and int(nat.lib().psignn_param_grad_size(1, 1)) != _FL_MIXED_UPD_NEU + 370 + 112:
        raise nat.NativeError("f_theta weight layout changed: update engine._FL_* offsets")
    wf = torch.zeros(n, dtype=torch.float32, device=device)
    blocks = [("phi_to", _FL_PHI_TO), ("phi_from", _FL_PHI_FROM)] + ([("phi_neumann", _FL_MIXED_PHI_NEU)] if mixed else [])
    for m, o in blocks:
        blk = torch.cat([g(f"{m}.mlp.mlp.0.weight"), g(f"{m}.mlp.mlp.0.bias"), g(f"{m}.mlp.mlp.2.weight"), g(f"{m}.mlp.mlp.2.bias")])
        wf[o:o + blk.numel()] = blk
    if mixed:
        blk = torch.cat([g(f"update_neumann.mlp.{q}") for q in ("0.weight", "0.bias", "2.weight", "2.bias")])
        wf[_FL_MIXED_UPD_NEU:_FL_MIXED_UPD_NEU + blk.numel()] = blk
    wg = torch.cat([g(f"{m}.mlp.0.{q}") for m in ("z_k", "r_k", "correction") for q in ("weight", "bias")])
    return wf, wg


def unpack_dsgps_grads(flat, mixed):
    """{state_dict name: gradient} from the flat buffer of ``psignn_dsgps_step_backward``."""
    base = int(nat.lib().psignn_param_grad_size(int(mixed), 1))
    out = {}
    for k, t in unpack_param_grads(flat[:base], 1, mixed).items():
        if k.startswith(("phi_to_list.0.", "phi_from_list.0.")):
            out[k.replace("_list.0.", ".")] = t
        elif k.startswith(("phi_neumann.", "update_neumann.")):
            out[k] = t
    cat = 3 * D + (3 if mixed else 2)
    o = base
    for m in ("z_k", "r_k", "correction"):
        out[f"{m}.mlp.0.weight"] = flat[o:o + D * cat].reshape(D, cat)
        o += D * cat
        out[f"{m}.mlp.0.bias"] = flat[o:o + D]
        o += D
    return out


def dsgps_step_backward(plan: "MeshPlan", wf, wg, h, prb, w, nrm=None):
    """({name: grad}, w^T dh'/dh) of one DS-GPS update (caller's numbering; mixed plans need the unit normals)."""
    hc, wc = _f32c(h), _f32c(w)
    l = nat.lib()
    mixed = nrm is not None
    grad = torch.empty(int(l.psignn_dsgps_grad_size(int(mixed))), dtype=torch.float32, device=hc.device)
    out = torch.empty_like(hc)
    if getattr(plan, "_dswork", None) is None:
        plan._dswork = torch.empty(int(l.psignn_dsgps_step_backward_workspace_floats(plan.handle)), dtype=torch.float32,
                                   device=hc.device)
    with torch.cuda.device(hc.device):
        nat.check(l.psignn_dsgps_step_backward(plan.handle, nat.ptr(wf), nat.ptr(wg), nat.ptr(hc), nat.ptr(_f32c(prb)),
                                               nat.ptr(None if nrm is None else _f32c(nrm)), nat.ptr(wc), nat.ptr(grad),
                                               nat.ptr(out), nat.ptr(plan._dswork), nat.stream_ptr(hc.device)),
                  "psignn_dsgps_step_backward")
    return unpack_dsgps_grads(grad, mixed), out


# f_theta base layout with three node inputs (csrc/common.h WLayout<3>): shared 64 | phi_to 350 | phi_from 350 | update 450 | fold
_DSS_PHI_TO, _DSS_PHI_FROM, _DSS_PSI = 64, 414, 764


def pack_dss_train(sd, t, device):
    """Update t's modules in the f_theta weight layout for ``psignn_dss_step_backward``: the (10, 21) first Phi layers padded
    to (10, 23) (edge-feature weight in column 22, the plan carries the scalar feature in the third attr column), Psi in
    the update slots.  Assembled on the device (it runs once per update in the backward pass)."""
    n = int(nat.lib().psignn_dss_grad_size())
    wf = torch.zeros(n, dtype=torch.float32, device=device)
    g = lambda k: sd[k].detach().to(device, torch.float32)
    for name, o in ((f"phi_to_list.{t}", _DSS_PHI_TO), (f"phi_from_list.{t}", _DSS_PHI_FROM)):
        w1 = g(f"{name}.mlp.mlp.0.weight")
        w1p = torch.zeros(D, 2 * D + 3, dtype=torch.float32, device=device)
        w1p[:, :2 * D], w1p[:, 2 * D + 2] = w1[:, :2 * D], w1[:, 2 * D]
        blk = torch.cat([w1p.reshape(-1), g(f"{name}.mlp.mlp.0.bias"), g(f"{name}.mlp.mlp.2.weight").reshape(-1),
                         g(f"{name}.mlp.mlp.2.bias")])
        wf[o:o + blk.numel()] = blk
    psi = f"psi_list.{t}.mlp.mlp"
    blk = torch.cat([g(f"{psi}.0.weight").reshape(-1), g(f"{psi}.0.bias"), g(f"{psi}.2.weight").reshape(-1), g(f"{psi}.2.bias")])
    wf[_DSS_PSI:_DSS_PSI + blk.numel()] = blk
    return wf


def unpack_dss_grads(flat, t):
    out = {}
    for name, o in ((f"phi_to_list.{t}", _DSS_PHI_TO), (f"phi_from_list.{t}", _DSS_PHI_FROM)):
        w1 = flat[o:o + D * (2 * D + 3)].reshape(D, 2 * D + 3)
        out[f"{name}.mlp.mlp.0.weight"] = torch.cat([w1[:, :2 * D], w1[:, 2 * D + 2:2 * D + 3]], dim=1)
        o += D * (2 * D + 3)
        out[f"{name}.mlp.mlp.0.bias"] = flat[o:o + D]
        out[f"{name}.mlp.mlp.2.weight"] = flat[o + D:o + D + D * D].reshape(D, D)
        out[f"{name}.mlp.mlp.2.bias"] = flat[o + D + D * D:o + 2 * D + D * D]
    o, cat = _DSS_PSI, 3 * D + 3
    psi = f"psi_list.{t}.mlp.mlp"
    out[f"{psi}.0.weight"] = flat[o:o + D * cat].reshape(D, cat)
    out[f"{psi}.0.bias"] = flat[o + D * cat:o + D * cat + D]
    o += D * cat + D
    out[f"{psi}.2.weight"] = flat[o:o + D * D].reshape(D, D)
    out[f"{psi}.2.bias"] = flat[o + D * D:o + D * D + D]
    return out


def dss_step_backward(plan: "MeshPlan", wf_t, t, alpha, h, bprime_norm, w):
    """({name: grad}, w^T dh'/dh) of DSS update t (caller's numbering)."""
    hc, wc = _f32c(h), _f32c(w)
    l = nat.lib()
    grad = torch.empty(int(l.psignn_dss_grad_size()), dtype=torch.float32, device=hc.device)
    out = torch.empty_like(hc)
    if getattr(plan, "_dsswork", None) is None:
        plan._dsswork = torch.empty(int(l.psignn_dss_step_backward_workspace_floats(plan.handle)), dtype=torch.float32,
                                    device=hc.device)
    with torch.cuda.device(hc.device):
        nat.check(l.psignn_dss_step_backward(plan.handle, nat.ptr(wf_t), float(alpha), nat.ptr(hc), nat.ptr(_f32c(bprime_norm)),
                                             nat.ptr(wc), nat.ptr(grad), nat.ptr(out), nat.ptr(plan._dsswork),
                                             nat.stream_ptr(hc.device)), "psignn_dss_step_backward")
    return unpack_dss_grads(grad, t), out


def pack_dss(sd, k, device=None) -> torch.Tensor:
    """Flat per-step weight buffer of the DSS kernels from a ``DeepStatisticalSolver`` state_dict
    (dirichlet/dss/model.py:33-55; layout in csrc/dss_tile.hip)."""
    m = lambda n: sd[n].detach().to("cpu", torch.float32)
    t = lambda a: a.t().contiguous().reshape(-1)
    z20 = torch.zeros(2 * D)
    steps = []
    for s in range(k):
        Wt, Wf = m(f"phi_to_list.{s}.mlp.mlp.0.weight"), m(f"phi_from_list.{s}.mlp.mlp.0.weight")
        if Wt.shape != (D, 2 * D + 1) or m(f"psi_list.{s}.mlp.mlp.0.weight").shape != (D, 3 * D + 3):
            raise nat.NativeError("DSS kernels are built for latent_dim = 10, a scalar edge feature and a 3-wide node input")
        steps += [t(Wt[:, D:2 * D]), t(Wf[:, D:2 * D]), t(Wt[:, :D]), t(Wf[:, :D]),
                  z20, Wt[:, 2 * D], z20, Wf[:, 2 * D],
                  m(f"phi_to_list.{s}.mlp.mlp.0.bias"), m(f"phi_from_list.{s}.mlp.mlp.0.bias"),
                  t(m(f"phi_to_list.{s}.mlp.mlp.2.weight")), m(f"phi_to_list.{s}.mlp.mlp.2.bias"),
                  t(m(f"phi_from_list.{s}.mlp.mlp.2.weight")), m(f"phi_from_list.{s}.mlp.mlp.2.bias"),
                  t(m(f"psi_list.{s}.mlp.mlp.0.weight")), m(f"psi_list.{s}.mlp.mlp.0.bias"),
                  t(m(f"psi_list.{s}.mlp.mlp.2.weight")), m(f"psi_list.{s}.mlp.mlp.2.bias")]
    flat = torch.cat([p.reshape(-1) for p in steps]).contiguous()
    if flat.numel() != int(nat.lib().psignn_dss_weights_size(int(k))):
        raise nat.NativeError(f"packed DSS weight length {flat.numel()} != native layout")
    return flat if device is None else flat.to(device)


def dss_forward(plan: "MeshPlan", wflat, bprime_norm, k: int, alpha: float):
    """H_k of ``DeepStatisticalSolver.inference`` (model.py:97-120) from H_0 = 0."""
    nat.require_cuda(bprime_norm, "b_prime_norm")
    bc = _f32c(bprime_norm)
    out = torch.empty((plan.N, D), dtype=torch.float32, device=bc.device)
    work = torch.empty(23 * plan.N, dtype=torch.float32, device=bc.device)
    with torch.cuda.device(bc.device):
        nat.check(nat.lib().psignn_dss_forward(plan.handle, nat.ptr(wflat), int(k), float(alpha), nat.ptr(bc), nat.ptr(out),
                                               nat.ptr(work), nat.stream_ptr(bc.device)), "psignn_dss_forward")
    return out


def dss_step_p(plan: "MeshPlan", wflat, t: int, alpha: float, hp, bprime_p):
    """DSS update t, state and b'_norm in plan order."""
    out = torch.empty_like(hp)
    with torch.cuda.device(hp.device):
        nat.check(nat.lib().psignn_dss_step_p(plan.handle, nat.ptr(wflat), int(t), float(alpha), nat.ptr(_f32c(hp)),
                                              nat.ptr(bprime_p), nat.ptr(out), nat.stream_ptr(hp.device)), "psignn_dss_step_p")
    return out


def unpack_param_grads(flat, n_layers=1, mixed=False):
    """Name the entries of a flat parameter gradient (layout = leading section of ``pack_weights``): the shared modules,
    then every layer's ``phi_to_list.k`` / ``phi_from_list.k`` / ``update_list.k`` (layer k's section starts k layer sizes
    after layer 0's), then, mixed family, ``phi_neumann`` / ``update_neumann`` behind the last layer."""
    if not 1 <= int(n_layers) <= 64:
        raise nat.NativeError(f"n_layers = {n_layers} is out of range")
    l = nat.lib()
    size = int(l.psignn_param_grad_size(int(mixed), int(n_layers)))
    lsz = int(l.psignn_param_grad_size(int(mixed), 2)) - int(l.psignn_param_grad_size(int(mixed), 1))
    if flat.numel() != size:
        raise nat.NativeError(f"flat gradient has {flat.numel()} entries, expected {size}")
    p = 3 if mixed else 2
    cat, ein = 3 * D + p, 2 * D + 3
    out, o = {}, 0

    def take(name, *shape):
        nonlocal o
        n = 1
        for k in shape:
            n *= k
        out[name] = flat[o:o + n].reshape(shape)
        o += n
    take("laynorm.weight", D)
    take("laynorm.bias", D)
    take("alpha.0.weight", 1, cat)
    take("alpha.0.bias", 1)
    for k in range(int(n_layers)):
        o = 64 + k * lsz
        for phi in ("phi_to_list", "phi_from_list"):
            take(f"{phi}.{k}.mlp.mlp.0.weight", D, ein)
            take(f"{phi}.{k}.mlp.mlp.0.bias", D)
            take(f"{phi}.{k}.mlp.mlp.2.weight", D, D)
            take(f"{phi}.{k}.mlp.mlp.2.bias", D)
        take(f"update_list.{k}.mlp.0.weight", D, cat)
        take(f"update_list.{k}.mlp.0.bias", D)
        take(f"update_list.{k}.mlp.2.weight", D, D)
        take(f"update_list.{k}.mlp.2.bias", D)
    if mixed:
        o = 64 + int(n_layers) * lsz   # behind the last layer (its fold slots included)
        take("phi_neumann.mlp.mlp.0.weight", D, ein)
        take("phi_neumann.mlp.mlp.0.bias", D)
        take("phi_neumann.mlp.mlp.2.weight", D, D)
        take("phi_neumann.mlp.mlp.2.bias", D)
        take("update_neumann.mlp.0.weight", D, 2 * D + p + 2)
        take("update_neumann.mlp.0.bias", D)
        take("update_neumann.mlp.2.weight", D, D)
        take("update_neumann.mlp.2.bias", D)
    return out


def mlp2_backward(x, gy, w1, b1, w2, need_gx=True):
    """Backward of ``mlp2``: (gx | None, gW1, gb1, gW2, gb2)."""
    xc, gc = _f32c(x), _f32c(gy)
    n, din = xc.shape
    hid, dout = w1.shape[0], w2.shape[0]
    l = nat.lib()
    gx = torch.empty_like(xc) if need_gx else None
    gflat = torch.empty(hid * din + hid + dout * hid + dout, dtype=torch.float32, device=xc.device)
    work = torch.empty(int(l.psignn_mlp2_backward_workspace_floats(n)), dtype=torch.float32, device=xc.device)
    with torch.cuda.device(xc.device):
        nat.check(l.psignn_mlp2_backward(nat.ptr(xc), nat.ptr(gc), n, din, hid, dout, nat.ptr(_f32c(w1)),
                                         nat.ptr(_f32c(b1)), nat.ptr(_f32c(w2)), nat.ptr(gx), nat.ptr(gflat),
                                         nat.ptr(work), nat.stream_ptr(xc.device)), "psignn_mlp2_backward")
    o1, o2, o3 = hid * din, hid * din + hid, hid * din + hid + dout * hid
    return gx, gflat[:o1].reshape(hid, din), gflat[o1:o2], gflat[o2:o3].reshape(dout, hid), gflat[o3:]


class _MLP2Fn(torch.autograd.Function):
    """mlp2 with its HIP backward, for the training path (encoder / decoder terms of the loss)."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2):
        ctx.save_for_backward(x, w1, b1, w2)
        return mlp2(x, w1, b1, w2, b2)

    @staticmethod
    def backward(ctx, gy):
        x, w1, b1, w2 = ctx.saved_tensors
        gx, g1, gb1, g2, gb2 = mlp2_backward(x, gy.contiguous(), w1, b1, w2, need_gx=ctx.needs_input_grad[0])
        return gx, g1, gb1, g2, gb2


def mlp2_autograd(x, w1, b1, w2, b2):
    if torch.is_grad_enabled() and any(t.requires_grad for t in (x, w1, b1, w2, b2)):
        return _MLP2Fn.apply(x, w1, b1, w2, b2)
    return mlp2(x, w1, b1, w2, b2)


def residual_t(plan: "MeshPlan", a_ij, r):
    """A^T r (backward of ``residual`` w.r.t. u); a_ij in the caller's edge order."""
    rc, ac = _f32c(r).reshape(-1), _f32c(a_ij).reshape(-1)
    if ac.numel() != plan.E:
        raise nat.NativeError(f"a_ij has {ac.numel()} entries, the plan {plan.E} edges")
    out = torch.empty_like(rc)
    with torch.cuda.device(rc.device):
        nat.check(nat.lib().psignn_residual_t(plan.handle, nat.ptr(ac), nat.ptr(rc), nat.ptr(out),
                                              nat.stream_ptr(rc.device)), "psignn_residual_t")
    return out.reshape(-1, 1)


class _ResidualFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, y, plan, a_ij):
        ctx.plan, ctx.a_ij = plan, a_ij
        return residual(plan, u, y)

    @staticmethod
    def backward(ctx, gr):
        return residual_t(ctx.plan, ctx.a_ij, gr.contiguous()), None, None, None


def residual_autograd(plan, u, y, a_ij):
    if torch.is_grad_enabled() and u.requires_grad:
        return _ResidualFn.apply(u, y, plan, a_ij)
    return residual(plan, u, y)


def mlp2(x, w1, b1, w2, b2):
    """relu(x W1^T + b1) W2^T + b2 for the tiny encoder/decoder MLPs (model.py:370-392)."""
    nat.require_cuda(x, "x")
    xc = _f32c(x)
    n, din = xc.shape
    hid, dout = w1.shape[0], w2.shape[0]
    out = torch.empty((n, dout), dtype=torch.float32, device=xc.device)
    with torch.cuda.device(xc.device):
        nat.check(nat.lib().psignn_mlp2(nat.ptr(xc), n, din, hid, dout, nat.ptr(_f32c(w1)), nat.ptr(_f32c(b1)),
                                        nat.ptr(_f32c(w2)), nat.ptr(_f32c(b2)), nat.ptr(out),
                                        nat.stream_ptr(xc.device)), "psignn_mlp2")
    return out


def residual(plan: MeshPlan, u, y):
    """A u - y with A = COO(edge_index, a_ij) including the diagonal (model.py:157-167)."""
    uc, yc = _f32c(u).reshape(-1), _f32c(y).reshape(-1)
    out = torch.empty_like(uc)
    with torch.cuda.device(uc.device):
        nat.check(nat.lib().psignn_residual(plan.handle, nat.ptr(uc), nat.ptr(yc), nat.ptr(out),
                                            nat.stream_ptr(uc.device)), "psignn_residual")
    return out.reshape(-1, 1)


# ---------------------------------------------------------------------------------------------
# device Broyden
# ---------------------------------------------------------------------------------------------
TRACE_BUDGET_BYTES = 8 << 30  # keep every iterate only while (thr+2)*N*d*4 stays under this


LIN_NEUMANN = ("direct", "stored")


JAC_BACKWARD = ("gather", "tiled")


def check_jac_backward(value):
    """``"gather"`` / ``"tiled"`` as given; ValueError for anything else (a host check: nothing is allocated)."""
    if not isinstance(value, str) or value not in JAC_BACKWARD:
        raise ValueError(f"jac_backward must be one of {JAC_BACKWARD}, got {value!r}")
    return value


BW_SOLVERS = (None, "gmres")


def check_bw_solver(value, m=None, bw_thres=None):
    """The ``bw_solver`` config value as given: ``None`` (the implicit backward runs ``config["solver"]``, the reference's route)
    or ``"gmres"`` (restarted GMRES on the adjoint system, ``DeviceGmres.solve_adjoint``); NativeError naming the accepted
    values for anything else.  With ``m`` and ``bw_thres``: the restart length ``bw_gmres_m`` must be an int in 2..``bw_thres``.
    A host check: nothing is allocated."""
    if value is not None and not (isinstance(value, str) and value in BW_SOLVERS):
        raise nat.NativeError(f"bw_solver must be one of {BW_SOLVERS}, got {value!r}")
    if m is not None:
        if isinstance(m, bool) or not isinstance(m, int) or not 2 <= m <= int(bw_thres):
            raise nat.NativeError(f"bw_gmres_m must be an int in 2..bw_thres (= {bw_thres}), got {m!r}")
    return value


def check_bw_gmres_lockstep(value, bw_solver):
    """The ``bw_gmres_lockstep`` config value as a bool: the replicas of a ``DataParallel(replicas=R)`` step solve their GMRES
    adjoint systems in lockstep (``gmres_solve_adjoint_batch``).  It needs ``bw_solver = "gmres"``: NativeError naming both keys
    otherwise.  A host check: nothing is allocated."""
    if not isinstance(value, bool):
        raise nat.NativeError(f"bw_gmres_lockstep must be a bool, got {value!r}")
    if value and bw_solver != "gmres":
        raise nat.NativeError(f'bw_gmres_lockstep = True needs bw_solver = "gmres" (bw_solver is {bw_solver!r})')
    return value


def check_bw_gmres_aug(augment, stall, bw_solver, m):
    """The ``bw_gmres_augment`` / ``bw_gmres_stall`` config values as ``(int, float)`` (None: the default, 0 / 0.5): corrections the
    GMRES adjoint solve keeps between restart cycles, an int in 0..min(``m`` - 1, 8) with ``m`` = ``bw_gmres_m``, and its stall ratio,
    a float in (0, 1] (``DeviceGmresAug.solve_adjoint``).  Both need ``bw_solver = "gmres"``: NativeError naming the keys otherwise.
    A host check: nothing is allocated."""
    if bw_solver != "gmres":
        raise nat.NativeError(f'bw_gmres_augment / bw_gmres_stall need bw_solver = "gmres" (bw_solver is {bw_solver!r})')
    a = 0 if augment is None else augment
    if isinstance(a, bool) or not isinstance(a, int) or not 0 <= a <= min(int(m) - 1, AUGMENT_MAX):
        raise nat.NativeError(f"bw_gmres_augment must be an int in 0..min(bw_gmres_m - 1, {AUGMENT_MAX}) = "
                              f"{min(int(m) - 1, AUGMENT_MAX)}, got {augment!r}")
    st = 0.5 if stall is None else stall
    if isinstance(st, bool) or not isinstance(st, (int, float)) or not 0.0 < float(st) <= 1.0:   # (a NaN is not)
        raise nat.NativeError(f"bw_gmres_stall must be a float in (0, 1], got {stall!r}")
    return a, float(st)


def check_lin_neumann(value):
    """``"direct"`` / ``"stored"`` as given; ValueError for anything else (a host check: nothing is allocated)."""
    if not isinstance(value, str) or value not in LIN_NEUMANN:
        raise ValueError(f"lin_neumann / neumann must be one of {LIN_NEUMANN}, got {value!r}")
    return value


class Linearization:
    """Stored linearisation of a FixedPointMap at one state (psignn_lin_* in include/psignn_hip.h).

    ``neumann`` (mixed family; ignored for dirichlet plans): ``"direct"`` -- the tiles holding Neumann nodes run the direct
    JVP kernel and ``vjp_p`` the tiled VJP, both at a copy of the state kept by the build; ``"stored"`` -- the Neumann rows are
    stored like every other row: ``jvp_p`` is one linear operator on all tiles and ``vjp_p`` its exact transpose, no state
    copy.  ``neumann_stored`` tells which form the handle holds."""

    def __init__(self, fmap, neumann="direct"):
        neumann = check_lin_neumann(neumann)
        nat.require_default_width(getattr(fmap, "width", D), "Linearization")
        if not fmap.can_linearize():
            raise nat.NativeError("linearize_p: tiled plans (dirichlet family: single-layer blocks); use jvp_p otherwise")
        self.fmap = fmap
        h = C.c_void_p()
        with torch.cuda.device(fmap.weights.flat.device):
            if neumann == "stored":
                nat.check(nat.lib().psignn_lin_create_opts(C.byref(h), fmap.plan.handle, 1), "psignn_lin_create_opts")
            else:
                nat.check(nat.lib().psignn_lin_create(C.byref(h), fmap.plan.handle), "psignn_lin_create")
        self.handle = h
        self.bytes = int(nat.lib().psignn_lin_bytes(h))
        self.neumann_stored = bool(nat.lib().psignn_lin_neumann_stored(h))

    def build(self, Hp):
        fm = self.fmap
        _, prbp, nrmp = fm._p
        Hc = _f32c(Hp)
        with torch.cuda.device(Hc.device):
            nat.check(nat.lib().psignn_lin_build(self.handle, nat.ptr(fm.weights.flat), fm.weights.n_layers, nat.ptr(Hc),
                                                 nat.ptr(prbp), nat.ptr(nrmp), nat.stream_ptr(Hc.device)), "psignn_lin_build")
        return self

    def jvp_p(self, Vp, out=None):
        """J_f(H) Vp for the H of the last ``build`` (plan order); ``out`` as in FixedPointMap.jvp_p."""
        fm = self.fmap
        Vc = _f32c(Vp)
        if out is None:
            out = torch.empty_like(Vc)
        elif out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != Vc.numel():
            raise nat.NativeError("jvp_p: out must be a contiguous float32 tensor of the state's size")
        with torch.cuda.device(Vc.device):
            nat.check(nat.lib().psignn_lin_jvp(self.handle, nat.ptr(fm.weights.flat), fm.weights.n_layers, nat.ptr(Vc),
                                               nat.ptr(out), nat.stream_ptr(Vc.device)), "psignn_lin_jvp")
        return out

    def vjp_p(self, Wp, out=None):
        """Wp^T J_f(H) for the H of the last ``build`` (plan order): the exact transpose of ``jvp_p`` (same stored masks and
        per-node records); the same product as ``FixedPointMap.vjp_p`` at that H up to fp32 summation order.  ``out`` as in
        ``jvp_p``."""
        fm = self.fmap
        Wc = _f32c(Wp)
        if out is None:
            out = torch.empty_like(Wc)
        elif out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != Wc.numel():
            raise nat.NativeError("vjp_p: out must be a contiguous float32 tensor of the state's size")
        with torch.cuda.device(Wc.device):
            nat.check(nat.lib().psignn_lin_vjp(self.handle, nat.ptr(fm.weights.flat), fm.weights.n_layers, nat.ptr(Wc),
                                               nat.ptr(out),
                                               nat.ptr(fm.plan.workspace() if fm.plan.mixed and not self.neumann_stored else None),
                                               nat.stream_ptr(Wc.device)),
                      "psignn_lin_vjp")
        return out

    def close(self):
        if self.handle is not None:
            nat.lib().psignn_lin_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# element type of the stored Broyden pairs -> ``history`` of psignn_broyden_create_opts
_HISTORY_CODES = {torch.float32: 0, torch.bfloat16: 1}


def history_code(history_dtype) -> int:
    """0 for ``torch.float32`` (the default), 1 for ``torch.bfloat16``; any other dtype raises ValueError (on the host, before
    anything is allocated)."""
    if history_dtype not in _HISTORY_CODES:
        raise ValueError(f"Broyden history dtype {history_dtype!r}: torch.float32 or torch.bfloat16")
    return _HISTORY_CODES[history_dtype]


class DeviceBroyden:
    def __init__(self, plan=None, threshold=50, keep_trace=False, n_elems=None, seq_len=D, device=None, shard_elems=0,
                 history_dtype=torch.float32, width=None):
        """``width``: the latent width of the maps this solver will serve (default: the default width; a plan-less solver is flat
        over its ``n_elems`` and takes any ``seq_len``).  The solver is made by that width's library and refuses a map of another.

        ``shard_elems`` > 0: the solver will run inside ``broyden_solve_batch`` with others; its reduction shapes are sized
        for the whole shard (sum of N * d), and its single-mesh solves give the same bits as the batched ones.

        ``history_dtype``: element type of the stored rank-one pairs U_j, V_j.  ``torch.bfloat16`` halves their memory and the
        bytes every iteration streams (``psignn_broyden_create_opts``, history = 1): each pair is rounded to bf16 when it is
        written and the new pair's derived values use the rounded one; iterate, update and arithmetic stay fp32.  Such a solver
        is never batched (``shard_batchable`` is False)."""
        hist = history_code(history_dtype)
        h = C.c_void_p()
        self.width = D if width is None else nat.check_width(width)
        self.plan = plan
        self.threshold = int(threshold)
        self.keep_trace = bool(keep_trace)
        self.history_dtype = history_dtype
        self.device = plan.device if plan is not None else device
        with torch.cuda.device(self.device):
            if hist:
                self._check(self.lib.psignn_broyden_create_opts(
                    C.byref(h), plan.handle if plan is not None else None, 0 if plan is not None else int(n_elems),
                    0 if plan is not None else int(seq_len), self.threshold, int(keep_trace), int(shard_elems), hist),
                    "psignn_broyden_create_opts")
                self.M = plan.N * self.width if plan is not None else int(n_elems)
            elif plan is not None:
                self._check(self.lib.psignn_broyden_create_for_batch(C.byref(h), plan.handle, self.threshold, int(keep_trace),
                                                                     int(shard_elems)), "psignn_broyden_create_for_batch")
                self.M = plan.N * self.width
            else:
                self._check(self.lib.psignn_broyden_create_n(C.byref(h), int(n_elems), int(seq_len), self.threshold,
                                                            int(keep_trace)), "psignn_broyden_create_n")
                self.M = int(n_elems)
        self.handle = h
        self._fin = weakref.finalize(self, self.lib.psignn_broyden_destroy, h)

    width = D   # (class default: a solver object filled in by hand around a native handle is a default-width one)

    @property
    def lib(self):
        """The library this solver was made by: its latent width's."""
        return nat.lib(self.width)

    def _check(self, rc, what=""):
        nat.check(rc, what, self.lib)

    def _same_width(self, fmap):
        if getattr(fmap, "lib", None) is not self.lib:
            raise nat.NativeError(f"solver of latent_dim {self.width} was handed a map of latent_dim {getattr(fmap, 'width', '?')}")

    def close(self):
        self._fin()

    @property
    def nbytes(self):
        return int(self.lib.psignn_broyden_bytes(self.handle))

    def set_stop_mode(self, stop_mode: str):
        """"rel" (default, every call site of the reference) or "abs" (solver.py:116,140,174)."""
        if stop_mode not in ("rel", "abs"):
            raise nat.NativeError(f"stop_mode {stop_mode!r}: 'rel' or 'abs'")
        self.stop_mode = stop_mode
        self._check(self.lib.psignn_broyden_set_stop_mode(self.handle, int(stop_mode == "abs")), "psignn_broyden_set_stop_mode")

    def _result(self, info, rel, abs_, result):
        n_it = info.n_iter
        low = float(info.lowest_abs if getattr(self, "stop_mode", "rel") == "abs" else info.lowest)
        out = {"nstep": int(info.nstep), "n_iter": int(n_it), "lowest": low,
               "prot_break": bool(info.prot_break), "stop_reason": int(info.stop_reason)}
        # reference pads both traces to threshold+1 entries with the lowest values (solver.py:195-197)
        rel_l = list(rel[:n_it]) + [float(info.lowest)] * (self.threshold + 1 - n_it)
        abs_l = list(abs_[:n_it]) + [float(info.lowest_abs)] * (self.threshold + 1 - n_it)
        out["rel_trace"], out["abs_trace"], out["result"] = rel_l, abs_l, result
        return out

    def solve(self, fmap: FixedPointMap, eps, poll_every=8):
        self._same_width(fmap)
        result = torch.empty_like(fmap.h0)
        info = nat.SolveInfo()
        rel = (C.c_double * self.threshold)()
        abs_ = (C.c_double * self.threshold)()
        with torch.cuda.device(self.device):
            self._check(self.lib.psignn_broyden_solve(
                self.handle, nat.ptr(fmap.weights.flat), fmap.weights.n_layers, nat.ptr(fmap.h0), nat.ptr(fmap.prb),
                nat.ptr(fmap.nrm), float(eps), int(poll_every), nat.ptr(result), C.byref(info), rel, abs_,
                nat.stream_ptr(self.device)), "psignn_broyden_solve")
        return self._result(info, rel, abs_, result)

    def solve_adjoint(self, fmap: FixedPointMap, h_star, grad, eps, poll_every=8, lin=None):
        """y = J_f(h*)^T y + grad, y_0 = 0, entirely on the device (VJP kernel inside the Broyden loop).  ``lin``: a Linearization
        of ``fmap`` built at h* (plan order, on this solver's plan); the loop then applies ``lin.vjp_p`` and ``h_star`` is not read."""
        nat.require_default_width(self.width, "solve_adjoint")
        self._same_width(fmap)
        hs, gr = _f32c(h_star), _f32c(grad)
        result = torch.empty_like(gr)
        info = nat.SolveInfo()
        rel = (C.c_double * self.threshold)()
        abs_ = (C.c_double * self.threshold)()
        with torch.cuda.device(self.device):
            if lin is not None:
                self._check(self.lib.psignn_broyden_solve_adjoint_lin(
                    self.handle, lin.handle, nat.ptr(fmap.weights.flat), fmap.weights.n_layers, nat.ptr(gr), float(eps),
                    int(poll_every), nat.ptr(result), C.byref(info), rel, abs_, nat.stream_ptr(self.device)),
                    "psignn_broyden_solve_adjoint_lin")
                return self._result(info, rel, abs_, result)
            self._check(self.lib.psignn_broyden_solve_adjoint(
                self.handle, nat.ptr(fmap.weights.flat), fmap.weights.n_layers, nat.ptr(hs), nat.ptr(fmap.prb),
                nat.ptr(fmap.nrm), nat.ptr(gr), float(eps), int(poll_every), nat.ptr(result), C.byref(info), rel, abs_,
                nat.stream_ptr(self.device)), "psignn_broyden_solve_adjoint")
        return self._result(info, rel, abs_, result)

    def iterate(self, i, like):
        dst = torch.empty_like(like)
        with torch.cuda.device(self.device):
            self._check(self.lib.psignn_broyden_get_iterate(self.handle, int(i), nat.ptr(dst),
                                                           nat.stream_ptr(self.device)), "psignn_broyden_get_iterate")
        return dst

    def pair(self, j, like, which="U"):
        """Stored rank-one pair j of the last solve (``U_j`` / ``V_j``; the reference's ``Us[..., j]`` / ``VTs[:, j]``,
        utilities/solver.py:190-191) or, ``which="update"``, the current update vector (``j`` ignored); caller's numbering."""
        dst = torch.empty_like(like)
        with torch.cuda.device(self.device):
            self._check(self.lib.psignn_broyden_get_pair(self.handle, int(j), {"U": 0, "V": 1, "update": 2, "parta": 3}[which], nat.ptr(dst),
                                                        nat.stream_ptr(self.device)), "psignn_broyden_get_pair")
        return dst

    def _armijo_step(self, f, phi0, lib, sp, like):
        """Step length of the reference's line search (line_search / scalar_search_armijo, utilities/solver.py:20-94) for
        the current update direction: backtracking on phi(s) = |f(x + s u) - (x + s u)|^2 with phi'(0) taken as -phi(0),
        c1 = 1e-4, first trial s = 1, then the minimiser of the quadratic through (0, 1), then cubic interpolation through
        the last two trials, safeguarded to shrink by at least 4 % and at most 50 % per round, given up below s = 1e-2
        (-> s = 1).  Like the reference, the quadratic trial is never tested against the Armijo condition itself.
        Returns (s, f(x + s u) if it was evaluated at that s else None, phi(s) or None)."""
        c1, amin, der0 = 1e-4, 1e-2, -phi0
        cache = {}

        def phi(s):
            xt = torch.empty_like(like)
            self._check(lib.psignn_broyden_ext_trial_x(self.handle, float(s), nat.ptr(xt), sp), "ext_trial_x")
            fx = _f32c(f(xt.clone()))
            g = fx - xt
            val = float(g.norm()) ** 2 if bool(torch.isfinite(g).all()) else float("inf")
            cache["s"], cache["fx"], cache["phi"] = s, fx, val
            return val

        def accept(s, val):
            return val <= phi0 + c1 * s * der0

        s0, p0 = 1.0, phi(1.0)
        if accept(s0, p0):
            return s0, cache["fx"], p0
        s1 = -der0 * s0 ** 2 / 2.0 / (p0 - phi0 - der0 * s0)
        p1 = phi(s1)
        while s1 > amin:
            den = s0 ** 2 * s1 ** 2 * (s1 - s0)
            r0, r1 = p0 - phi0 - der0 * s0, p1 - phi0 - der0 * s1
            ca = (s0 ** 2 * r1 - s1 ** 2 * r0) / den
            cb = (-s0 ** 3 * r1 + s1 ** 3 * r0) / den
            s2 = (-cb + abs(cb ** 2 - 3.0 * ca * der0) ** 0.5) / (3.0 * ca)
            p2 = phi(s2)
            if accept(s2, p2):
                return s2, cache["fx"], p2
            if (s1 - s2) > s1 / 2.0 or (1.0 - s2 / s1) < 0.96:
                s2 = s1 / 2.0
            s0, s1, p0, p1 = s1, s2, p1, p2
        # no admissible step: s = 1 (solver.py:85-93; f there is re-evaluated unless the last trial was at s = 1)
        return 1.0, (cache["fx"] if cache["s"] == 1.0 else None), None

    def solve_callable(self, f, x0, eps, ls=False):
        """Generic f (any Python callable on device tensors): one f call per iteration from the host (ls=True: plus the
        trial evaluations of the Armijo line search)."""
        x0c = _f32c(x0)
        lib, sp = self.lib, nat.stream_ptr(self.device)
        with torch.cuda.device(self.device):
            fx = _f32c(f(x0c))
            self._check(lib.psignn_broyden_ext_begin(self.handle, nat.ptr(x0c), nat.ptr(fx), sp), "ext_begin")
            done = C.c_int(0)
            xn = torch.empty_like(x0c)
            phi_cur = float((fx - x0c).norm()) ** 2 if ls else 0.0
            self.ls_steps = []
            for _ in range(self.threshold):
                if ls:
                    s, fx_s, phi_s = self._armijo_step(f, phi_cur, lib, sp, x0c)
                    self.ls_steps.append(s)
                    if s != 1.0:
                        self._check(lib.psignn_broyden_ext_scale_step(self.handle, float(s), sp), "ext_scale_step")
                    self._check(lib.psignn_broyden_ext_next_x(self.handle, nat.ptr(xn), sp), "ext_next_x")
                    fx = fx_s if fx_s is not None else _f32c(f(xn.clone()))
                    phi_cur = phi_s if phi_s is not None else float((fx - xn).norm()) ** 2
                    self._check(lib.psignn_broyden_ext_update(self.handle, nat.ptr(fx), float(eps), C.byref(done), sp),
                              "ext_update")
                    if done.value:
                        break
                    continue
                self._check(lib.psignn_broyden_ext_next_x(self.handle, nat.ptr(xn), sp), "ext_next_x")
                fx = _f32c(f(xn.clone()))
                self._check(lib.psignn_broyden_ext_update(self.handle, nat.ptr(fx), float(eps), C.byref(done), sp),
                          "ext_update")
                if done.value:
                    break
            result = torch.empty_like(x0c)
            info = nat.SolveInfo()
            rel = (C.c_double * self.threshold)()
            abs_ = (C.c_double * self.threshold)()
            self._check(lib.psignn_broyden_ext_finish(self.handle, nat.ptr(result), C.byref(info), rel, abs_, sp),
                      "ext_finish")
        return self._result(info, rel, abs_, result)


class _ShardCall:
    """ctypes marshalling of one lockstep solve of n meshes (the three ``*_batch`` wrappers below): the check that all meshes share
    one packed weight buffer (``what`` names the solve in its message), the info array, one ``c_double`` trace row per mesh with
    the pointer-to-pointer arrays the library fills them through, pointer arrays, and the zip into per-mesh result dicts."""

    def __init__(self, what, weights, info_type, trace_lens):
        self.n, self.w0 = len(weights), weights[0]
        if any(w is not self.w0 and w.flat.data_ptr() != self.w0.flat.data_ptr() for w in weights):
            raise nat.NativeError(f"{what}: all meshes must share one packed weight buffer")
        self.infos = (info_type * self.n)()
        self.rel = [(C.c_double * k)() for k in trace_lens]
        self.abs_ = [(C.c_double * k)() for k in trace_lens]

    def arr(self, ptrs):
        return (C.c_void_p * self.n)(*ptrs)

    def handles(self, objs):
        return self.arr([o.handle.value for o in objs])

    def tensors(self, ts):
        return self.arr([nat.ptr(t) for t in ts])

    def traces(self):
        """(rel, abs) as ``double* const*``."""
        dpp = lambda rows: (C.POINTER(C.c_double) * self.n)(*[C.cast(r, C.POINTER(C.c_double)) for r in rows])
        return dpp(self.rel), dpp(self.abs_)

    def collect(self, result_of, results):
        """``[result_of[i](info, rel, abs_, result) for mesh i]``."""
        return [f(self.infos[i], self.rel[i], self.abs_[i], results[i]) for i, f in enumerate(result_of)]


def shard_batchable(solvers) -> bool:
    """Whether ``broyden_solve_batch`` takes these solvers together: tiled plans of one family (all dirichlet or all mixed) and one
    size class (``psignn_broyden_batchable``).  A host-side decision -- real errors of the batched solve still raise."""
    n = len(solvers)
    if n == 0:
        return False
    if any(s.lib is not solvers[0].lib for s in solvers):   # solvers of different latent widths never share a shard
        return False
    arr = (C.c_void_p * n)(*[s.handle.value for s in solvers])
    return bool(solvers[0].lib.psignn_broyden_batchable(n, arr))


def broyden_solve_batch(solvers, fmaps, eps, poll_every=8):
    """One lockstep device solve of several independent meshes (``psignn_broyden_solve_batch``): ``solvers[i]`` is a
    ``DeviceBroyden`` of ``fmaps[i].plan``; all dirichlet or all mixed.  Returns the list of per-mesh result dicts of
    ``DeviceBroyden.solve`` -- each bit-identical to solving that mesh alone."""
    n = len(solvers)
    if n == 0:
        return []
    if len(fmaps) != n:
        raise nat.NativeError("one FixedPointMap per solver")
    call = _ShardCall("batched solve", [f.weights for f in fmaps], nat.SolveInfo, [s.threshold for s in solvers])
    w0 = call.w0
    for s, f in zip(solvers, fmaps):
        if s.plan is not f.plan:
            raise nat.NativeError("batched solve: solver and map were built from different plans")
        if s.lib is not w0.lib or f.lib is not w0.lib:
            raise nat.NativeError("batched solve: solvers and maps of one latent width only")
    dev = solvers[0].device
    results = [torch.empty_like(f.h0) for f in fmaps]
    with torch.cuda.device(dev):
        nat.check(w0.lib.psignn_broyden_solve_batch(
            n, call.handles(solvers), nat.ptr(w0.flat), w0.n_layers, call.tensors([f.h0 for f in fmaps]),
            call.tensors([f.prb for f in fmaps]), call.tensors([f.nrm for f in fmaps]) if w0.mixed else None,
            float(eps), int(poll_every), call.tensors(results), call.infos, *call.traces(), nat.stream_ptr(dev)),
            "psignn_broyden_solve_batch", w0.lib)
    return call.collect([s._result for s in solvers], results)


def adjoint_batchable(solvers, lins) -> bool:
    """Whether ``broyden_solve_adjoint_batch`` takes these solvers and linearisations together
    (``psignn_broyden_adjoint_batchable``): all that ``shard_batchable`` asks of the solvers, and every ``lins[i]`` was made for
    ``solvers[i]``'s plan, has been built and holds a form the batched transposed product takes (dirichlet; mixed only with
    ``neumann="stored"``).  A host-side decision -- real errors of the batched solve still raise."""
    if any(getattr(s, "width", D) != D for s in solvers):   # the adjoint solves exist at the default width only
        return False
    n = len(solvers)
    if n == 0 or len(lins) != n or any(l is None or l.handle is None for l in lins):
        return False
    sv = (C.c_void_p * n)(*[s.handle.value for s in solvers])
    lv = (C.c_void_p * n)(*[l.handle.value for l in lins])
    return bool(nat.lib().psignn_broyden_adjoint_batchable(n, sv, lv))


def broyden_solve_adjoint_batch(solvers, lins, grads, eps, poll_every=8):
    """One lockstep device solve of the adjoint fixed points y_i = J_i^T y_i + grads[i] of several independent meshes
    (``psignn_broyden_solve_adjoint_lin_batch``): ``solvers[i]`` is a ``DeviceBroyden`` of the plan ``lins[i]`` was made for
    (created with ``shard_elems``), ``lins[i]`` a ``Linearization`` built at mesh i's H*.  ``grads`` and the results are in the
    caller's numbering.  Returns the list of per-mesh result dicts of ``DeviceBroyden.solve_adjoint`` -- each bit-identical to
    ``solvers[i].solve_adjoint(..., lin=lins[i])`` on that mesh alone.  A shard ``adjoint_batchable`` does not take raises
    ``NativeError`` with nothing launched."""
    n = len(solvers)
    if n == 0:
        return []
    if len(lins) != n or len(grads) != n:
        raise nat.NativeError("one Linearization and one gradient per solver")
    call = _ShardCall("batched adjoint solve", [l.fmap.weights for l in lins], nat.SolveInfo, [s.threshold for s in solvers])
    w0 = call.w0
    for s, l in zip(solvers, lins):
        if s.plan is not l.fmap.plan:
            raise nat.NativeError("batched adjoint solve: solver and linearisation were made for different plans")
    dev = solvers[0].device
    gr = [_f32c(g) for g in grads]
    results = [torch.empty_like(g) for g in gr]
    with torch.cuda.device(dev):
        nat.check(nat.lib().psignn_broyden_solve_adjoint_lin_batch(
            n, call.handles(solvers), call.handles(lins), nat.ptr(w0.flat), w0.n_layers, call.tensors(gr), float(eps),
            int(poll_every), call.tensors(results), call.infos, *call.traces(), nat.stream_ptr(dev)),
            "psignn_broyden_solve_adjoint_lin_batch")
    return call.collect([s._result for s in solvers], results)


# ---------------------------------------------------------------------------------------------
# Picard / Anderson on the device (csrc/fpiter.hip)
# ---------------------------------------------------------------------------------------------
class DeviceFixedPointIter:
    """Vector work, norms, stop tests and the small bordered solve of ``forward_iteration`` / ``anderson``
    (utilities/solver.py:301-341, :215-293) on the device.  The caller evaluates f between the calls; nothing is read back
    per iteration unless asked (``poll``)."""

    def __init__(self, n_elems, device, m=2, threshold=50, keep_trace=False, width=None, shard_elems=None):
        """``width``: the latent width of the map being iterated (default: the default width): the state lives in that
        width's library, like the map's other handles.  The arithmetic is flat over ``n_elems``.
        ``shard_elems``: the summed length of the shard this handle will share an ``anderson_solve_batch`` /
        ``picard_solve_batch`` call with (``psignn_fpiter_create_for_batch``: the vector width follows the shard, and the handle
        holds the rows the lockstep solves keep per mesh); ``None``: a handle sized for itself."""
        h = C.c_void_p()
        self.lib = nat.lib(D if width is None else width)
        self.device, self.M, self.m = device, int(n_elems), int(m)
        self.threshold, self.keep_trace = int(threshold), bool(keep_trace)
        self.shard_elems = None if shard_elems is None else int(shard_elems)
        with torch.cuda.device(device):
            if self.shard_elems is None:
                nat.check(self.lib.psignn_fpiter_create(C.byref(h), self.M, self.m, self.threshold, int(self.keep_trace)),
                          "psignn_fpiter_create", self.lib)
            else:
                nat.check(self.lib.psignn_fpiter_create_for_batch(C.byref(h), self.M, self.m, self.threshold, int(self.keep_trace),
                                                                  self.shard_elems), "psignn_fpiter_create_for_batch", self.lib)
        self.handle = h
        self._fin = weakref.finalize(self, self.lib.psignn_fpiter_destroy, h)

    def close(self):
        self._fin()

    def _sp(self):
        return nat.stream_ptr(self.device)

    def poll(self):
        d = C.c_int(0)
        nat.check(self.lib.psignn_fpiter_poll(self.handle, C.byref(d), self._sp()), "psignn_fpiter_poll", self.lib)
        return bool(d.value)

    # Picard
    def picard_begin(self, x0):
        nat.check(self.lib.psignn_picard_begin(self.handle, nat.ptr(x0), self._sp()), "psignn_picard_begin", self.lib)

    def picard_current(self, like):
        x = torch.empty_like(like)
        nat.check(self.lib.psignn_picard_current_x(self.handle, nat.ptr(x), self._sp()), "psignn_picard_current_x", self.lib)
        return x

    def picard_update(self, fx, eps):
        nat.check(self.lib.psignn_picard_update(self.handle, nat.ptr(fx), float(eps), None, self._sp()), "psignn_picard_update", self.lib)

    # Anderson
    def anderson_begin(self, x0, f0, f1, lam, beta, stop_abs):
        nat.check(self.lib.psignn_anderson_begin(self.handle, nat.ptr(x0), nat.ptr(f0), nat.ptr(f1), float(lam), float(beta),
                                                  int(stop_abs), self._sp()), "psignn_anderson_begin", self.lib)

    def anderson_next(self, like):
        x = torch.empty_like(like)
        nat.check(self.lib.psignn_anderson_next_x(self.handle, nat.ptr(x), self._sp()), "psignn_anderson_next_x", self.lib)
        return x

    def anderson_update(self, fx, eps):
        nat.check(self.lib.psignn_anderson_update(self.handle, nat.ptr(fx), float(eps), None, self._sp()),
                  "psignn_anderson_update", self.lib)

    def finish(self, like):
        result = torch.empty_like(like)
        info = nat.SolveInfo()
        n = self.threshold + 2
        rel, abs_, low = (C.c_double * n)(), (C.c_double * n)(), (C.c_int32 * n)()
        nat.check(self.lib.psignn_fpiter_finish(self.handle, nat.ptr(result), C.byref(info), rel, abs_, low, self._sp()),
                  "psignn_fpiter_finish", self.lib)
        return self._result(info, rel, abs_, low, result)

    @staticmethod
    def _result(info, rel, abs_, low, result):
        k = int(info.n_iter)
        return {"result": result, "n_iter": k, "nstep": int(info.nstep), "lowest": float(info.lowest),
                "lowest_abs": float(info.lowest_abs), "stop_reason": int(info.stop_reason),
                "rel_trace": list(rel[:k]), "abs_trace": list(abs_[:k]), "low_idx": list(low[:k])}

    def iterate(self, i, like):
        dst = torch.empty_like(like)
        nat.check(self.lib.psignn_fpiter_get_iterate(self.handle, int(i), nat.ptr(dst), self._sp()), "psignn_fpiter_get_iterate", self.lib)
        return dst


def check_fp_lockstep(value, solver, accepted):
    """The ``fp_lockstep`` config value as a bool: the meshes of a shard (``batch.solve_shard_batched``, the replicas of a
    ``DataParallel(replicas=R)`` step) run their Anderson / Picard forward solves in lockstep (``anderson_solve_batch`` /
    ``picard_solve_batch``).  It needs ``solver`` to be one of ``accepted`` (``utilities.solver.anderson`` and
    ``forward_iteration``, handed in by the model): NativeError naming both keys otherwise.  A host check: nothing is allocated."""
    if not isinstance(value, bool):
        raise nat.NativeError(f"fp_lockstep must be a bool, got {value!r}")
    if value and not any(solver is a for a in accepted):
        raise nat.NativeError(f"fp_lockstep = True needs solver in ({', '.join(a.__name__ for a in accepted)}) "
                              f"(solver is {getattr(solver, '__name__', solver)!r})")
    return value


def fpiter_batchable(iters, fmaps) -> bool:
    """Whether ``anderson_solve_batch`` / ``picard_solve_batch`` take these handles and maps together
    (``psignn_fpiter_batchable``): tiled plans of one family, every ``iters[i]`` made with ``shard_elems`` for the length of
    ``fmaps[i]``'s plan, one vector width, one ``m``, one threshold, no kept trace; and, on the host, one latent width and
    single-layer weights.  A host-side decision -- real errors of the lockstep solves still raise."""
    n = len(iters)
    if n == 0 or len(fmaps) != n:
        return False
    lib = iters[0].lib
    if any(it.lib is not lib for it in iters) or any(f.lib is not lib or f.weights.n_layers != 1 for f in fmaps):
        return False
    hv = (C.c_void_p * n)(*[it.handle.value for it in iters])
    pv = (C.c_void_p * n)(*[f.plan.handle.value for f in fmaps])
    return bool(lib.psignn_fpiter_batchable(n, hv, pv))


def _fp_shard_call(what, iters, fmaps):
    """Marshalling shared by the two lockstep fixed-point solves; NativeError (nothing launched) for a shard that is not batchable."""
    n = len(iters)
    if len(fmaps) != n:
        raise nat.NativeError("one FixedPointMap per handle")
    call = _ShardCall(what, [f.weights for f in fmaps], nat.SolveInfo, [it.threshold + 2 for it in iters])
    if not fpiter_batchable(iters, fmaps):
        raise nat.NativeError(f"{what}: handles / maps are not batchable (engine.fpiter_batchable): tiled plans of one family, "
                              "single-layer weights, handles made with shard_elems for their plans, one vector width, one m, one "
                              "threshold, no kept trace")
    plans = call.arr([f.plan.handle.value for f in fmaps])
    return call, plans


def anderson_solve_batch(iters, fmaps, eps, lam=1e-4, beta=1.0, stop_mode="rel", poll_every=8):
    """One lockstep Anderson solve of several independent meshes (``psignn_anderson_solve_batch``) from x0 = each map's
    ``h0``: ``iters[i]`` is a ``DeviceFixedPointIter(fmaps[i].plan.N * width, ..., shard_elems=...)``.  Returns one dict per mesh
    with the fields of ``DeviceFixedPointIter.finish`` (result in the caller's numbering) -- each bit-identical to driving that
    handle through ``anderson_begin / anderson_next / anderson_update / finish`` around ``fmap.fp`` on that mesh alone.  A shard
    ``fpiter_batchable`` does not take raises ``NativeError`` with nothing launched."""
    if stop_mode not in ("rel", "abs"):
        raise ValueError(f"stop_mode {stop_mode!r}")
    if len(iters) == 0:
        return []
    call, plans = _fp_shard_call("lockstep anderson solve", iters, fmaps)
    w0, dev = call.w0, iters[0].device
    results = [torch.empty_like(f.h0) for f in fmaps]
    lows = [(C.c_int32 * (it.threshold + 2))() for it in iters]
    lpp = (C.POINTER(C.c_int32) * call.n)(*[C.cast(r, C.POINTER(C.c_int32)) for r in lows])
    with torch.cuda.device(dev):
        nat.check(w0.lib.psignn_anderson_solve_batch(
            call.n, call.handles(iters), plans, nat.ptr(w0.flat), w0.n_layers, call.tensors([f.h0 for f in fmaps]),
            call.tensors([f.prb for f in fmaps]), call.tensors([f.nrm for f in fmaps]) if w0.mixed else None, float(lam), float(beta),
            int(stop_mode == "abs"), float(eps), int(poll_every), call.tensors(results), call.infos, *call.traces(), lpp,
            nat.stream_ptr(dev)), "psignn_anderson_solve_batch", w0.lib)
    return [DeviceFixedPointIter._result(call.infos[i], call.rel[i], call.abs_[i], lows[i], results[i]) for i in range(call.n)]


def picard_solve_batch(iters, fmaps, eps, poll_every=8):
    """One lockstep Picard solve z <- f(z) of several independent meshes (``psignn_picard_solve_batch``) from z0 = each map's
    ``h0``; handles and result dicts as ``anderson_solve_batch`` (``low_idx`` is all zeros: Picard keeps no lowest iterate)."""
    if len(iters) == 0:
        return []
    call, plans = _fp_shard_call("lockstep picard solve", iters, fmaps)
    w0, dev = call.w0, iters[0].device
    results = [torch.empty_like(f.h0) for f in fmaps]
    with torch.cuda.device(dev):
        nat.check(w0.lib.psignn_picard_solve_batch(
            call.n, call.handles(iters), plans, nat.ptr(w0.flat), w0.n_layers, call.tensors([f.h0 for f in fmaps]),
            call.tensors([f.prb for f in fmaps]), call.tensors([f.nrm for f in fmaps]) if w0.mixed else None, float(eps),
            int(poll_every), call.tensors(results), call.infos, *call.traces(), nat.stream_ptr(dev)),
            "psignn_picard_solve_batch", w0.lib)
    zeros = [0] * (max(it.threshold for it in iters) + 2)
    return [DeviceFixedPointIter._result(call.infos[i], call.rel[i], call.abs_[i], zeros, results[i]) for i in range(call.n)]


# ---------------------------------------------------------------------------------------------
# GMRES on the device (csrc/krylov.hip)
# ---------------------------------------------------------------------------------------------
GMRES_STOPS = ("budget", "tolerance", "stagnation")   # stop_reason of psignn_gmres_adjoint_info_t


class DeviceGmres:
    """Krylov workspace of ``newton_krylov``: the basis is a torch tensor (rows are handed to the JVP kernel as views),
    everything else -- Gram-Schmidt sweeps, Hessenberg / Givens least squares, stop flag -- lives in the library.
    ``solve_adjoint`` runs the restarted solve of the implicit backward's adjoint system on the same workspace.
    ``shard_elems``: the summed length of the shard this handle will share a ``gmres_solve_adjoint_batch`` call with
    (``psignn_gmres_create_for_batch``: the vector width follows the shard); ``None``: a handle sized for itself."""

    def __init__(self, n_elems, device, m_max, shard_elems=None):
        self.M, self.m, self.device = int(n_elems), int(m_max), device
        self.shard_elems = None if shard_elems is None else int(shard_elems)
        self.ld = (self.M + 63) // 64 * 64
        self.V = torch.empty((self.m + 1, self.ld), dtype=torch.float32, device=device)
        h = C.c_void_p()
        with torch.cuda.device(device):
            if self.shard_elems is None:
                nat.check(nat.lib().psignn_gmres_create(C.byref(h), self.M, self.ld, self.m, nat.ptr(self.V)), "psignn_gmres_create")
            else:   # sized for a shard of ``gmres_solve_adjoint_batch``: one vector width for all its handles
                nat.check(nat.lib().psignn_gmres_create_for_batch(C.byref(h), self.M, self.ld, self.m, nat.ptr(self.V),
                                                                  self.shard_elems), "psignn_gmres_create_for_batch")
        self.handle = h
        self._fin = weakref.finalize(self, nat.lib().psignn_gmres_destroy, h)

    def close(self):
        self._fin()
        self._work = self._work_key = None

    _work = _work_key = None

    @property
    def nbytes(self):
        """Solver state in bytes: the (m + 1) basis vectors, what the library allocated for the handle (``psignn_gmres_bytes``: the
        dot partials, one row per block, so this differs between the two vector widths) and the adjoint solve's workspace, if one
        has been made."""
        return (self.V.numel() * 4 + int(nat.lib().psignn_gmres_bytes(self.handle))
                + (self._work.numel() * 4 if self._work is not None else 0))

    def solve_adjoint(self, fmap, h_star, grad, eps, max_products, lin=None, poll_every=8):
        """y = J_f(h*)^T y + grad by restarted GMRES (restart length = this object's ``m_max``), y_0 = 0, entirely on the device
        (psignn_gmres_solve_adjoint / _lin in include/psignn_hip.h).  ``eps`` is a bound on the Broyden solver's measure
        |f(y) - y| / (|f(y)| + 1e-9); the solve also ends when a cycle no longer halves it (the working precision is reached) or
        when ``max_products`` transposed products are spent.  ``lin``: a Linearization of ``fmap`` built at h*; the products
        then are ``lin.vjp_p`` and ``h_star`` is not read.  Returns the dict of ``DeviceBroyden.solve_adjoint``: ``result`` (the
        caller's numbering, the iterate with the lowest measure), ``nstep`` = products spent, ``lowest``, ``rel_trace`` /
        ``abs_trace`` with one entry per cycle, plus ``n_cycles``, ``stop`` (one of ``GMRES_STOPS``) and ``n_reorth``."""
        nat.require_default_width(getattr(fmap, "width", D), "solve_adjoint")
        plan, nl = fmap.plan, fmap.weights.n_layers
        if plan.N * D != self.M:
            raise nat.NativeError(f"DeviceGmres of {self.M} elements was handed a map of {plan.N * D}")
        hs, gr = _f32c(h_star), _f32c(grad)
        result = torch.empty_like(gr)
        info = nat.GmresAdjointInfo()
        cap = int(max_products) // 2 + 3
        rel, abs_ = (C.c_double * cap)(), (C.c_double * cap)()
        lib = nat.lib()
        with torch.cuda.device(self.device):
            self._workspace(plan, nl)
            if lin is not None:
                nat.check(lib.psignn_gmres_solve_adjoint_lin(
                    self.handle, lin.handle, nat.ptr(fmap.weights.flat), nl, nat.ptr(gr), float(eps), int(max_products),
                    int(poll_every), nat.ptr(self._work), nat.ptr(result), C.byref(info), rel, abs_, self._sp()),
                    "psignn_gmres_solve_adjoint_lin")
            else:
                nat.check(lib.psignn_gmres_solve_adjoint(
                    self.handle, plan.handle, nat.ptr(fmap.weights.flat), nl, nat.ptr(hs), nat.ptr(fmap.prb), nat.ptr(fmap.nrm),
                    nat.ptr(gr), float(eps), int(max_products), int(poll_every), nat.ptr(self._work), nat.ptr(result),
                    C.byref(info), rel, abs_, self._sp()), "psignn_gmres_solve_adjoint")
        return self._result(info, rel, abs_, result)

    def _workspace(self, plan, nl):
        """The adjoint solve's workspace for (plan, n_layers), kept between solves (call inside ``torch.cuda.device``)."""
        if self._work_key is None or self._work_key[0] is not plan or self._work_key[1] != nl:
            n = int(nat.lib().psignn_gmres_adjoint_workspace_floats(plan.handle, nl))
            if n < 0:
                raise nat.NativeError("psignn_gmres_adjoint_workspace_floats: bad plan or n_layers")
            self._work, self._work_key = torch.empty(n, dtype=torch.float32, device=self.device), (plan, nl)
        return self._work

    @staticmethod
    def _result(info, rel, abs_, result):
        n = min(int(info.cycles), len(rel))
        return {"result": result, "nstep": int(info.products), "lowest": float(info.lowest), "lowest_abs": float(info.lowest_abs),
                "rel_trace": list(rel[:n]), "abs_trace": list(abs_[:n]), "n_cycles": int(info.cycles),
                "stop": GMRES_STOPS[int(info.stop_reason)], "n_reorth": int(info.n_reorth), "prot_break": False}

    def row(self, j, shape):
        return self.V[j, :self.M].view(shape)

    def _sp(self):
        return nat.stream_ptr(self.device)

    def residual_norms(self, x, fx, g=None, neg_g=None):
        """(|fx - x|, |fx|) as the fp32 norms the reference reads back with .item(); optionally stores g and -g."""
        out = (C.c_double * 2)()
        nat.check(nat.lib().psignn_residual_norms(self.handle, nat.ptr(x), nat.ptr(fx), nat.ptr(g), nat.ptr(neg_g), out,
                                                  self._sp()), "psignn_residual_norms")
        return float(out[0]), float(out[1])

    def begin(self, b):
        nat.check(nat.lib().psignn_gmres_begin(self.handle, nat.ptr(b), self._sp()), "psignn_gmres_begin")

    def step(self, j, shift, eta, poll=False):
        d = C.c_int(0)
        nat.check(nat.lib().psignn_gmres_step(self.handle, int(j), float(shift), float(eta), C.byref(d) if poll else None,
                                              self._sp()), "psignn_gmres_step")
        return bool(d.value)

    def solution(self, base, scale, dst, k=0, info=False):
        inf = (C.c_double * 3)()
        nat.check(nat.lib().psignn_gmres_solution(self.handle, int(k), nat.ptr(base), float(scale), nat.ptr(dst),
                                                  inf if info else None, self._sp()), "psignn_gmres_solution")
        return (int(inf[0]), float(inf[1]), float(inf[2])) if info else None

    def reorth_count(self):
        """Arnoldi steps of the current solve whose second Gram-Schmidt pass ran."""
        n = C.c_int(0)
        nat.check(nat.lib().psignn_gmres_reorth_count(self.handle, C.byref(n), self._sp()), "psignn_gmres_reorth_count")
        return int(n.value)

    def history(self):
        h = (C.c_double * (self.m + 1))()
        nat.check(nat.lib().psignn_gmres_history(self.handle, h, self._sp()), "psignn_gmres_history")
        return list(h)


class DeviceGmresAug(DeviceGmres):
    """``DeviceGmres`` whose adjoint solves take augmented restarts (LGMRES) and a settable stall ratio (``psignn_gmres_create_aug``,
    ``psignn_gmres_solve_adjoint_opts`` / ``_lin_opts``; the method: the header of csrc/krylov_f64.hip, here with fp32 vectors).  The
    ring of ``augment + 1`` rows beside the basis is a torch tensor, like the basis; a solve keeps the ``augment`` newest corrections
    of its cycles and searches them in the last steps of the next cycle.  ``stall``: the solve ends on a cycle with ``not rel <=
    stall * prev_rel``; 0.5 is ``DeviceGmres``'s rule, 1.0 stops only when a cycle does not lower ``rel``.  ``augment=0, stall=0.5``
    launches the kernels of ``DeviceGmres`` and gives its bits.  A class of its own because the signatures of ``DeviceGmres`` are
    pinned.  The lockstep solve (``gmres_solve_adjoint_batch``) takes no options."""

    def __init__(self, n_elems, device, m_max, augment=0, shard_elems=None):
        self.augment = check_augment(augment, m_max, "DeviceGmresAug")
        self.M, self.m, self.device = int(n_elems), int(m_max), device
        self.shard_elems = None if shard_elems is None else int(shard_elems)
        if self.shard_elems is not None and self.shard_elems < self.M:
            raise nat.NativeError(f"DeviceGmresAug: shard_elems is the summed length of the shard, at least n_elems = {self.M}, "
                                  f"got {shard_elems}")
        self.ld = (self.M + 63) // 64 * 64
        self.V = torch.empty((self.m + 1, self.ld), dtype=torch.float32, device=device)
        self.Z = torch.zeros((self.augment + 1, self.ld), dtype=torch.float32, device=device) if self.augment else None
        h = C.c_void_p()
        with torch.cuda.device(device):
            nat.check(nat.lib().psignn_gmres_create_aug(C.byref(h), self.M, self.ld, self.m, nat.ptr(self.V), self.augment,
                                                        nat.ptr(self.Z), self.shard_elems or 0), "psignn_gmres_create_aug")
        self.handle = h
        self._fin = weakref.finalize(self, nat.lib().psignn_gmres_destroy, h)

    @property
    def nbytes(self):
        """``DeviceGmres.nbytes`` plus the ring."""
        return DeviceGmres.nbytes.fget(self) + (self.Z.numel() * 4 if self.Z is not None else 0)

    def solve_adjoint(self, fmap, h_star, grad, eps, max_products, lin=None, poll_every=8, augment=None, stall=0.5):
        """``DeviceGmres.solve_adjoint`` with ``augment`` (None: the handle's) and ``stall``.  The dict gains ``n_aug`` (the
        augmentation steps of the solve) and ``augment``."""
        opts = gmres64_opts(augment, stall, self.augment, "DeviceGmresAug.solve_adjoint", nat.GmresOpts)
        nat.require_default_width(getattr(fmap, "width", D), "solve_adjoint")
        plan, nl = fmap.plan, fmap.weights.n_layers
        if plan.N * D != self.M:
            raise nat.NativeError(f"DeviceGmresAug of {self.M} elements was handed a map of {plan.N * D}")
        hs, gr = _f32c(h_star), _f32c(grad)
        result = torch.empty_like(gr)
        info = nat.GmresInfo()
        cap = int(max_products) // 2 + 3
        rel, abs_ = (C.c_double * cap)(), (C.c_double * cap)()
        lib = nat.lib()
        with torch.cuda.device(self.device):
            self._workspace(plan, nl)
            if lin is not None:
                nat.check(lib.psignn_gmres_solve_adjoint_lin_opts(
                    self.handle, lin.handle, nat.ptr(fmap.weights.flat), nl, nat.ptr(gr), float(eps), int(max_products),
                    int(poll_every), C.byref(opts), nat.ptr(self._work), nat.ptr(result), C.byref(info), rel, abs_, self._sp()),
                    "psignn_gmres_solve_adjoint_lin_opts")
            else:
                nat.check(lib.psignn_gmres_solve_adjoint_opts(
                    self.handle, plan.handle, nat.ptr(fmap.weights.flat), nl, nat.ptr(hs), nat.ptr(fmap.prb), nat.ptr(fmap.nrm),
                    nat.ptr(gr), float(eps), int(max_products), int(poll_every), C.byref(opts), nat.ptr(self._work), nat.ptr(result),
                    C.byref(info), rel, abs_, self._sp()), "psignn_gmres_solve_adjoint_opts")
        out = self._result(info, rel, abs_, result)
        out["n_aug"], out["augment"] = int(info.n_aug), int(opts.augment)
        return out


def gmres_adjoint_batchable(solvers, lins) -> bool:
    """Whether ``gmres_solve_adjoint_batch`` takes these ``DeviceGmres`` handles and linearisations together
    (``psignn_gmres_adjoint_batchable``): one vector width and one restart length, every ``lins[i]`` built and of a form the batched
    transposed product takes (dirichlet; mixed only with ``neumann="stored"``), ``solvers[i]`` made for the length of ``lins[i]``'s
    plan, one family, single-layer blocks.  A host-side decision -- real errors of the batched solve still raise."""
    n = len(solvers)
    if n == 0 or len(lins) != n or any(l is None or l.handle is None for l in lins):
        return False
    if any(l.fmap.weights.n_layers != 1 for l in lins):   # the batched solve runs single-layer blocks
        return False
    sv = (C.c_void_p * n)(*[s.handle.value for s in solvers])
    lv = (C.c_void_p * n)(*[l.handle.value for l in lins])
    return bool(nat.lib().psignn_gmres_adjoint_batchable(n, sv, lv))


def gmres_solve_adjoint_batch(solvers, lins, grads, eps, max_products, poll_every=8):
    """One lockstep device solve of the adjoint systems y_i = J_i^T y_i + grads[i] of several independent meshes by restarted GMRES
    (``psignn_gmres_solve_adjoint_lin_batch``): ``solvers[i]`` is a ``DeviceGmres`` of the length of the plan ``lins[i]`` was made
    for (created with ``shard_elems``), ``lins[i]`` a ``Linearization`` built at mesh i's H*.  ``grads`` and the results are in the
    caller's numbering.  Returns the list of per-mesh result dicts of ``DeviceGmres.solve_adjoint`` -- each bit-identical to
    ``solvers[i].solve_adjoint(..., lin=lins[i])`` on that mesh alone, whatever ``poll_every``.  Each handle keeps its workspace, as
    in ``solve_adjoint``.  A shard ``gmres_adjoint_batchable`` does not take raises ``NativeError`` with nothing launched."""
    n = len(solvers)
    if n == 0:
        return []
    if len(lins) != n or len(grads) != n:
        raise nat.NativeError("one Linearization and one gradient per solver")
    if any(l is None or l.handle is None for l in lins):
        raise nat.NativeError("batched GMRES adjoint solve: every replica needs a Linearization")
    cap = int(max_products) // 2 + 3
    call = _ShardCall("batched GMRES adjoint solve", [l.fmap.weights for l in lins], nat.GmresAdjointInfo, [cap] * n)
    w0 = call.w0
    for s, l in zip(solvers, lins):
        if s.M != l.fmap.plan.N * D:
            raise nat.NativeError(f"batched GMRES adjoint solve: DeviceGmres of {s.M} elements was handed a linearisation of "
                                  f"{l.fmap.plan.N * D}")
    dev = solvers[0].device
    gr = [_f32c(g) for g in grads]
    results = [torch.empty_like(g) for g in gr]
    with torch.cuda.device(dev):
        works = [s._workspace(l.fmap.plan, w0.n_layers) for s, l in zip(solvers, lins)]
        nat.check(nat.lib().psignn_gmres_solve_adjoint_lin_batch(
            n, call.handles(solvers), call.handles(lins), nat.ptr(w0.flat), w0.n_layers, call.tensors(gr), float(eps),
            int(max_products), int(poll_every), call.tensors(works), call.tensors(results), call.infos, *call.traces(),
            nat.stream_ptr(dev)), "psignn_gmres_solve_adjoint_lin_batch")
    return call.collect([s._result for s in solvers], results)


# ---------------------------------------------------------------------------------------------
# reference solve of A u = y (csrc/poisson_cg.hip)
# ---------------------------------------------------------------------------------------------
def _f64_or_f32(t, name):
    """A float32 or float64 device tensor as a flat contiguous one plus its is-float64 flag (other dtypes go to float64)."""
    nat.require_cuda(t, name)
    if t.dtype not in (torch.float32, torch.float64):
        t = t.to(torch.float64)
    return t.reshape(-1).contiguous(), int(t.dtype == torch.float64)


def default_cg_max_iter(n_nodes: int) -> int:
    """max(1000, 20 ceil(sqrt(N))): Jacobi-PCG on 2-D P1 Poisson needs about 1/2 sqrt(kappa) ln(2 / tol) iterations with
    sqrt(kappa) ~ 0.64 sqrt(N) -- about 7 600 at 1M nodes and tol = 1e-10, so the cap leaves about 2.6x headroom."""
    return max(1000, 20 * int(np.ceil(np.sqrt(n_nodes))))


class PoissonCG:
    """Device-native solve of the discrete Poisson system ``A u = y`` of a plan's mesh: Jacobi-preconditioned conjugate gradient
    in float64 (``psignn_cg_*`` in include/psignn_hip.h) -- what ``scipy.sparse.linalg.spsolve`` is to ``data.hexmesh._solve``,
    at any size.  ``a_ij``: the (E,) or (E, 1) values in ``edge_index`` order, float32 (widened exactly) or float64; the
    handle keeps its own float64 copy.  Rows the plan flags as Dirichlet are fixed to ``y``; the others solve the lifted
    system.  Raises ``NativeError`` when the matrix is not symmetric with a positive diagonal on its free rows."""

    def __init__(self, plan: MeshPlan, a_ij):
        a, a64 = _f64_or_f32(a_ij, "a_ij")
        if a.numel() != plan.E:
            raise nat.NativeError(f"a_ij has {a.numel()} values, the plan {plan.E} edges")
        self.plan, self.N, self.device = plan, plan.N, plan.device
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            nat.check(nat.lib().psignn_cg_create(C.byref(h), plan.handle, nat.ptr(a), a64, nat.stream_ptr(self.device)),
                      "psignn_cg_create")
        self.handle = h
        self._fin = weakref.finalize(self, nat.lib().psignn_cg_destroy, h)

    def close(self):
        self._fin()
        self.handle = None

    def solve(self, y, x0=None, tol=1e-10, max_iter=None, poll_every=50):
        """``y``: (N,) or (N, 1), float32 or float64.  ``x0``: start on the free rows (default zeros).  Stops on
        ``|r| <= tol |b|`` (b: the lifted right-hand side on the free rows) or after ``max_iter`` iterations (default
        ``default_cg_max_iter(N)``).  Returns ``result`` (N, 1) float64 in the caller's numbering, ``n_iter``, ``converged``,
        ``rel`` (recurrence residual), ``true_rel`` (|(y - A x)_F| / |b| recomputed from the result), ``res_trace``
        (n_iter + 1 relative residuals), ``b_norm`` and ``sym_defect``.  Deterministic; ``poll_every`` (how often the host
        looks at the done flag) changes nothing in the result."""
        if self.handle is None:
            raise nat.NativeError("PoissonCG is closed")
        yc, y64 = _f64_or_f32(y, "y")
        if yc.numel() != self.N:
            raise nat.NativeError(f"y has {yc.numel()} entries, the plan {self.N} nodes")
        if max_iter is None:
            max_iter = default_cg_max_iter(self.N)
        max_iter = int(max_iter)
        x0c = None
        if x0 is not None:
            nat.require_cuda(x0, "x0")
            x0c = x0.to(torch.float64).reshape(-1).contiguous()
            if x0c.numel() != self.N:
                raise nat.NativeError(f"x0 has {x0c.numel()} entries, the plan {self.N} nodes")
        result = torch.empty((self.N, 1), dtype=torch.float64, device=self.device)
        info = nat.CgInfo()
        trace = (C.c_double * (max(max_iter, 0) + 1))()
        with torch.cuda.device(self.device):
            nat.check(nat.lib().psignn_cg_solve(self.handle, nat.ptr(yc), y64, nat.ptr(x0c), float(tol), max_iter, int(poll_every),
                                                nat.ptr(result), C.byref(info), trace, nat.stream_ptr(self.device)),
                      "psignn_cg_solve")
        n = int(info.n_iter)
        return {"result": result, "n_iter": n, "converged": bool(info.converged), "rel": float(info.rel),
                "true_rel": float(info.true_rel), "res_trace": list(trace[:n + 1]), "b_norm": float(info.b_norm),
                "sym_defect": float(info.sym_defect)}


def poisson_solve(batch, tol=1e-10, **kw):
    """``PoissonCG(plan_for(batch), batch.a_ij).solve(batch.y, tol=tol, **kw)``.  A union batch is one block-diagonal system."""
    cg = PoissonCG(plan_for(batch), batch.a_ij)
    try:
        return cg.solve(batch.y, tol=tol, **kw)
    finally:
        cg.close()


# ---------------------------------------------------------------------------------------------
# the forward path in float64 (csrc/fgnn_f64.hip, csrc/solver_f64.hip): the float64 fixed point h* on the device
# ---------------------------------------------------------------------------------------------
def _f64c(t, name):
    """A device tensor as a contiguous float64 one (float32 widens exactly)."""
    nat.require_cuda(t, name)
    return t.to(torch.float64).contiguous()


def pack_weights64(sd) -> torch.Tensor:
    """The ``deqdss.f.*`` tensors of a reference state dict as one flat float64 CPU tensor, in state-dict order with nothing
    padded, folded or transposed (layout: include/psignn_hip.h, "The forward path in float64"): laynorm, alpha, then per layer
    phi_to / phi_from / update, then (mixed) phi_neumann / update_neumann; each block weight, bias, weight, bias."""
    P = "deqdss.f."
    g = lambda k: sd[P + k].detach().to("cpu", torch.float64).reshape(-1)
    mlp = lambda prefix: [g(f"{prefix}.0.weight"), g(f"{prefix}.0.bias"), g(f"{prefix}.2.weight"), g(f"{prefix}.2.bias")]
    parts = [g("laynorm.weight"), g("laynorm.bias"), g("alpha.0.weight"), g("alpha.0.bias")]
    for l in range(n_layers_of(sd)):
        parts += mlp(f"phi_to_list.{l}.mlp.mlp") + mlp(f"phi_from_list.{l}.mlp.mlp") + mlp(f"update_list.{l}.mlp")
    if is_mixed_state_dict(sd):
        parts += mlp("phi_neumann.mlp.mlp") + mlp("update_neumann.mlp")
    return torch.cat(parts).contiguous()


class PackedWeights64:
    """Float64 weights of f for ``FixedPointMap64``.  Default latent width only: a state dict of another supported width raises
    the "forward inference only" ``NativeError`` of that width's library."""

    def __init__(self, sd, device=None):
        self.mixed = is_mixed_state_dict(sd)
        self.n_layers = n_layers_of(sd)
        self.width = width_of(sd)
        expect = nat.lib(self.width).psignn_f64_weights_size(int(self.mixed), self.n_layers)   # a width library: raises
        if sd["deqdss.f.alpha.0.weight"].numel() != 3 * self.width + (3 if self.mixed else 2):
            raise nat.NativeError("alpha gate width does not match the boundary-condition family")
        flat = pack_weights64(sd)
        if flat.numel() != expect:
            raise nat.NativeError(f"packed float64 weight length {flat.numel()} != native layout {expect}")
        self.flat = flat if device is None else flat.to(device)


def mlp2_64(x, w1, b1, w2, b2):
    """relu(x W1^T + b1) W2^T + b2 in float64 (``psignn_mlp2_f64``): the encoder / decoder of the float64 path.  Inputs of any
    float dtype are widened; the result is float64."""
    xc = _f64c(x, "x")
    if xc.dim() != 2 or w1.shape[1] != xc.shape[1] or w2.shape[1] != w1.shape[0]:
        raise nat.NativeError(f"mlp2_64: x {tuple(x.shape)}, W1 {tuple(w1.shape)}, W2 {tuple(w2.shape)} do not chain")
    n, din = xc.shape
    hid, dout = w1.shape[0], w2.shape[0]
    out = torch.empty((n, dout), dtype=torch.float64, device=xc.device)
    dv = lambda t: t.detach().to(xc.device, torch.float64).contiguous()
    w1, b1, w2, b2 = dv(w1), dv(b1), dv(w2), dv(b2)
    with torch.cuda.device(xc.device):
        nat.check(nat.lib().psignn_mlp2_f64(nat.ptr(xc), n, din, hid, dout, nat.ptr(w1), nat.ptr(b1), nat.ptr(w2), nat.ptr(b2),
                                            nat.ptr(out), nat.stream_ptr(xc.device)), "psignn_mlp2_f64")
    return out


def mlp2_64_backward(x, gy, w1, b1, w2, need_gx=True):
    """Backward of ``mlp2_64`` in float64 (``psignn_mlp2_f64_backward``): (gx | None, gW1, gb1, gW2, gb2), the tuple of
    ``mlp2_backward``.  Inputs of any float dtype are widened; per-chunk partials added in a fixed order, so deterministic."""
    xc, gc = _f64c(x, "x"), _f64c(gy, "gy")
    if (xc.dim() != 2 or gc.dim() != 2 or xc.shape[0] != gc.shape[0] or w1.shape[1] != xc.shape[1] or w2.shape[1] != w1.shape[0]
            or gc.shape[1] != w2.shape[0] or b1.numel() != w1.shape[0]):
        raise nat.NativeError(f"mlp2_64_backward: x {tuple(x.shape)}, gy {tuple(gy.shape)}, W1 {tuple(w1.shape)}, "
                              f"W2 {tuple(w2.shape)} do not chain")
    n, din = xc.shape
    hid, dout = w1.shape[0], w2.shape[0]
    l = nat.lib()
    nw = int(l.psignn_mlp2_f64_backward_workspace_doubles(n, din, hid, dout))
    if nw < 0:
        raise nat.NativeError(f"mlp2_64_backward: sizes {din} -> {hid} -> {dout} are out of range (at most 16 each)")
    dv = lambda t: t.detach().to(xc.device, torch.float64).contiguous()
    w1, b1, w2 = dv(w1), dv(b1), dv(w2)
    gx = torch.empty_like(xc) if need_gx else None
    gflat = torch.empty(hid * din + hid + dout * hid + dout, dtype=torch.float64, device=xc.device)
    work = torch.empty(nw, dtype=torch.float64, device=xc.device)
    with torch.cuda.device(xc.device):
        nat.check(l.psignn_mlp2_f64_backward(nat.ptr(xc), nat.ptr(gc), n, din, hid, dout, nat.ptr(w1), nat.ptr(b1), nat.ptr(w2),
                                             nat.ptr(gx), nat.ptr(gflat), nat.ptr(work), nw, nat.stream_ptr(xc.device)),
                  "psignn_mlp2_f64_backward")
    o1, o2, o3 = hid * din, hid * din + hid, hid * din + hid + dout * hid
    return gx, gflat[:o1].reshape(hid, din), gflat[o1:o2], gflat[o2:o3].reshape(dout, hid), gflat[o3:]


def unpack_param_grads64(flat, n_layers=1, mixed=False):
    """Name the entries of a flat float64 parameter gradient, the layout of ``pack_weights64`` (nothing padded, no fold slots):
    the names of ``unpack_param_grads``."""
    if not 1 <= int(n_layers) <= 64:
        raise nat.NativeError(f"n_layers = {n_layers} is out of range")
    p = 3 if mixed else 2
    cat, ein, ncat = 3 * D + p, 2 * D + 3, 2 * D + p + 2
    mlp = lambda prefix, k: [(f"{prefix}.0.weight", (D, k)), (f"{prefix}.0.bias", (D,)), (f"{prefix}.2.weight", (D, D)),
                             (f"{prefix}.2.bias", (D,))]
    items = [("laynorm.weight", (D,)), ("laynorm.bias", (D,)), ("alpha.0.weight", (1, cat)), ("alpha.0.bias", (1,))]
    for k in range(int(n_layers)):
        items += mlp(f"phi_to_list.{k}.mlp.mlp", ein) + mlp(f"phi_from_list.{k}.mlp.mlp", ein) + mlp(f"update_list.{k}.mlp", cat)
    if mixed:
        items += mlp("phi_neumann.mlp.mlp", ein) + mlp("update_neumann.mlp", ncat)
    size = sum(math.prod(shape) for _, shape in items)
    if flat.numel() != size:
        raise nat.NativeError(f"flat gradient has {flat.numel()} entries, expected {size}")
    out, o = {}, 0
    for name, shape in items:
        n = math.prod(shape)
        out[name] = flat[o:o + n].reshape(shape)
        o += n
    return out


class FixedPointMap64:
    """``H -> f(H, H_init, batch)`` in float64 on the device: (N, 10) float64 -> (N, 10) float64 in the caller's numbering, on
    tiled and untiled plans alike.  ``edge_attr``: the batch's (E, 3) array in ``edge_index`` order, float32 (widened exactly) or
    float64; the native handle keeps its own float64 copy in the plan's canonical order.  ``h_initial``, ``prb_data``,
    ``normals``: float32 (widened exactly) or float64.  ``jvp`` / ``vjp``: the float64 products ``J_f(H) V`` / ``J_f(H)^T W`` on
    the same handle (csrc/fgnn_f64_deriv.hip).  Shape and family mismatches raise ``NativeError`` before any native call."""

    def __init__(self, plan, weights64, h_initial, prb_data, edge_attr, normals=None):
        if plan.mixed != weights64.mixed:
            raise nat.NativeError("boundary-condition family of the weights and of the batch differ "
                                  f"(weights mixed={weights64.mixed}, batch mixed={plan.mixed})")
        if plan.mixed and normals is None:
            raise nat.NativeError("mixed problems need batch.unit_normal_vector")
        exp_p = 3 if plan.mixed else 2
        if (tuple(prb_data.shape) != (plan.N, exp_p) or tuple(h_initial.shape) != (plan.N, D)
                or tuple(edge_attr.shape) != (plan.E, 3) or (normals is not None and tuple(normals.shape) != (plan.N, 2))):
            raise nat.NativeError(f"shape mismatch: prb_data {tuple(prb_data.shape)}, h_initial {tuple(h_initial.shape)}, "
                                  f"edge_attr {tuple(edge_attr.shape)} for a plan of {plan.N} nodes and {plan.E} edges")
        self.plan, self.weights, self.device = plan, weights64, plan.device
        self.h0 = _f64c(h_initial, "h_initial")
        self.prb = _f64c(prb_data, "prb_data")
        self.nrm = None if normals is None or not plan.mixed else _f64c(normals, "normals")
        self.wflat = weights64.flat.to(self.device)
        ea, ea64 = _f64_or_f32(edge_attr, "edge_attr")
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            nat.check(nat.lib().psignn_f64_create(C.byref(h), plan.handle, nat.ptr(ea), ea64, nat.stream_ptr(self.device)),
                      "psignn_f64_create")
        self.handle = h
        self._deriv_work = {}   # transposed? -> workspace tensor of jvp / vjp, made on first use
        self._fin = weakref.finalize(self, nat.lib().psignn_f64_destroy, h)

    def close(self):
        self._fin()
        self.handle = None

    def _states(self, *named):
        """(tensor, name) pairs as float64 device tensors, None staying None; every shape is checked before any tensor is touched."""
        if self.handle is None:
            raise nat.NativeError("FixedPointMap64 is closed")
        for t, name in named:
            if t is not None and tuple(t.shape) != (self.plan.N, D):
                raise nat.NativeError(f"{name} has shape {tuple(t.shape)}, expected {(self.plan.N, D)}")
        return [None if t is None else _f64c(t, name) for t, name in named]

    def _state(self, H, name="H"):
        return self._states((H, name))[0]

    def __call__(self, H):
        Hc = self._state(H)
        out = torch.empty_like(Hc)
        with torch.cuda.device(self.device):
            nat.check(nat.lib().psignn_f64_forward(self.handle, nat.ptr(self.wflat), self.weights.n_layers, nat.ptr(Hc),
                                                   nat.ptr(self.h0), nat.ptr(self.prb), nat.ptr(self.nrm), nat.ptr(out),
                                                   nat.stream_ptr(self.device)), "psignn_f64_forward")
        return out

    def _work(self, transposed):
        """The workspace of a float64 product, kept on the map: ``psignn_f64_deriv_workspace_doubles`` doubles (None for 0)."""
        n = int(nat.lib().psignn_f64_deriv_workspace_doubles(self.handle, self.weights.n_layers, int(transposed)))
        if n < 0:
            raise nat.NativeError("psignn_f64_deriv_workspace_doubles refused the handle")
        have = self._deriv_work.get(transposed)
        if n and (have is None or have.numel() != n):   # made on first use; made again should the block's depth ever change
            have = self._deriv_work[transposed] = torch.empty(n, dtype=torch.float64, device=self.device)
        return (have if n else None), n

    def _work_both(self):
        """The workspace of a solve that runs either product: the larger of the two (``psignn_gmres64_solve_shifted``)."""
        a, b = self._work(False), self._work(True)
        return a if a[1] > b[1] else b

    def jvp(self, H, V):
        """``J_f(H) V`` in float64 (``psignn_f64_jvp``): H, V (N, 10), float32 (widened exactly) or float64; float64 comes out.
        Deterministic."""
        Hc, Vc = self._states((H, "H"), (V, "V"))
        out = torch.empty_like(Hc)
        work, n = self._work(False)
        with torch.cuda.device(self.device):
            nat.check(nat.lib().psignn_f64_jvp(self.handle, nat.ptr(self.wflat), self.weights.n_layers, nat.ptr(Hc), nat.ptr(self.h0),
                                               nat.ptr(self.prb), nat.ptr(self.nrm), nat.ptr(Vc), nat.ptr(out), nat.ptr(work), n,
                                               nat.stream_ptr(self.device)), "psignn_f64_jvp")
        return out

    def vjp(self, H, Wv, add=None):
        """``J_f(H)^T Wv`` in float64 (``psignn_f64_vjp``), plus ``add`` when given -- ``vjp(h_star, y, grad)`` is the map of the
        adjoint system ``y = J^T y + grad``.  Shapes (N, 10), float32 (widened exactly) or float64; float64 comes out.
        Deterministic."""
        Hc, Wc, Ac = self._states((H, "H"), (Wv, "Wv"), (add, "add"))
        out = torch.empty_like(Hc)
        work, n = self._work(True)
        with torch.cuda.device(self.device):
            nat.check(nat.lib().psignn_f64_vjp(self.handle, nat.ptr(self.wflat), self.weights.n_layers, nat.ptr(Hc), nat.ptr(self.h0),
                                               nat.ptr(self.prb), nat.ptr(self.nrm), nat.ptr(Wc), nat.ptr(Ac), nat.ptr(out),
                                               nat.ptr(work), n, nat.stream_ptr(self.device)), "psignn_f64_vjp")
        return out

    def param_vjp(self, H, Wv, with_init=True):
        """What ``loss.backward()`` leaves in the ``deqdss.f`` parameters for new_H = f(H) with cotangent Wv, in float64
        (``psignn_f64_param_vjp``; dirichlet/psignn/model.py:203-225, mixed likewise): ({name: float64 grad}, ``J_f(H)^T Wv``,
        ``Wv^T df/dH_init`` | None), the names those of ``FixedPointMap.param_vjp_init``.  H, Wv: (N, 10), float32 (widened exactly)
        or float64.  Both families, any depth, tiled or not; no atomics and a fixed summation order, so deterministic."""
        Hc, Wc = self._states((H, "H"), (Wv, "Wv"))
        l = nat.lib()
        nl, mixed = self.weights.n_layers, self.weights.mixed
        n = int(l.psignn_f64_param_vjp_workspace_doubles(self.handle, nl))
        if n < 0:
            raise nat.NativeError("psignn_f64_param_vjp_workspace_doubles refused the handle")
        work = self._deriv_work.get("param_vjp")
        if work is None or work.numel() != n:   # made on first use, like the products' workspaces
            work = self._deriv_work["param_vjp"] = torch.empty(n, dtype=torch.float64, device=self.device)
        grad = torch.empty(int(l.psignn_f64_weights_size(int(mixed), nl)), dtype=torch.float64, device=self.device)
        out = torch.empty_like(Hc)
        g_init = torch.empty_like(Hc) if with_init else None
        with torch.cuda.device(self.device):
            nat.check(l.psignn_f64_param_vjp(self.handle, nat.ptr(self.wflat), nl, nat.ptr(Hc), nat.ptr(self.h0), nat.ptr(self.prb),
                                             nat.ptr(self.nrm), nat.ptr(Wc), nat.ptr(grad), nat.ptr(out), nat.ptr(g_init),
                                             nat.ptr(work), n, nat.stream_ptr(self.device)), "psignn_f64_param_vjp")
        return unpack_param_grads64(grad, nl, mixed), out, g_init

    def vjp_backward(self, H, V, Gbar):
        """Backward of the VJP in float64 (``psignn_f64_vjp_backward``; jac_loss_estimate, dirichlet/psignn/model.py:416-435 with
        ``create_graph=True``): for ``psi = <Gbar, J_f(H)^T V>`` with Gbar constant, ({name: float64 d psi / d theta}, ``d psi / dH``,
        ``J_f(H)^T V``), the tuple and the names of ``FixedPointMap.vjp_backward``.  H, V, Gbar: (N, 10), float32 (widened exactly) or
        float64.  Both families, any depth, tiled or not; no atomics and a fixed summation order, so deterministic."""
        return self._vjp_backward(H, V, Gbar, False)[:3]

    def vjp_backward_init(self, H, V, Gbar):
        """``vjp_backward`` and ``d psi / dH_init`` as a fourth entry (``psignn_f64_vjp_backward_init``): the Dirichlet rows through
        which the Jacobian of a multi-layer dirichlet block depends on ``H_init``; exact zeros for every other block.  The first three
        entries have the bits of ``vjp_backward``."""
        return self._vjp_backward(H, V, Gbar, True)

    def _vjp_backward(self, H, V, Gbar, with_init):
        Hc, Vc, Gc = self._states((H, "H"), (V, "V"), (Gbar, "Gbar"))
        l = nat.lib()
        nl, mixed = self.weights.n_layers, self.weights.mixed
        n = int(l.psignn_f64_vjp_backward_workspace_doubles(self.handle, nl))
        if n < 0:
            raise nat.NativeError("psignn_f64_vjp_backward_workspace_doubles refused the handle")
        work = self._deriv_work.get("vjp_backward")
        if work is None or work.numel() != n:   # made on first use, like the products' workspaces
            work = self._deriv_work["vjp_backward"] = torch.empty(n, dtype=torch.float64, device=self.device)
        grad = torch.empty(int(l.psignn_f64_weights_size(int(mixed), nl)), dtype=torch.float64, device=self.device)
        dh, jtv = torch.empty_like(Hc), torch.empty_like(Hc)
        dinit = torch.empty_like(Hc) if with_init else None
        lead = (self.handle, nat.ptr(self.wflat), nl, nat.ptr(Hc), nat.ptr(self.h0), nat.ptr(self.prb), nat.ptr(self.nrm), nat.ptr(Vc),
                nat.ptr(Gc), nat.ptr(grad), nat.ptr(dh), nat.ptr(jtv))
        with torch.cuda.device(self.device):
            if with_init:
                nat.check(l.psignn_f64_vjp_backward_init(*lead, nat.ptr(dinit), nat.ptr(work), n, nat.stream_ptr(self.device)),
                          "psignn_f64_vjp_backward_init")
            else:
                nat.check(l.psignn_f64_vjp_backward(*lead, nat.ptr(work), n, nat.stream_ptr(self.device)), "psignn_f64_vjp_backward")
        return unpack_param_grads64(grad, nl, mixed), dh, jtv, dinit


class DeviceBroyden64:
    """Broyden root-find of ``f(x) - x`` in float64 with every scalar on the device (``psignn_broyden64_*``): the reference's
    recurrences (``ls=False``, stop mode ``rel``) on a ``FixedPointMap64``.  The pairs are stored in float64,
    ``2 * threshold * N * 10 * 8`` bytes; creation raises ``NativeError`` naming that size when the device cannot hold them."""

    def __init__(self, fmap64, threshold):
        if getattr(fmap64, "handle", None) is None:
            raise nat.NativeError("DeviceBroyden64 needs an open FixedPointMap64")
        self.fmap, self.threshold, self.device = fmap64, int(threshold), fmap64.device
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            nat.check(nat.lib().psignn_broyden64_create(C.byref(h), fmap64.handle, self.threshold), "psignn_broyden64_create")
        self.handle = h
        self._fin = weakref.finalize(self, nat.lib().psignn_broyden64_destroy, h)

    def close(self):
        self._fin()
        self.handle = None

    @property
    def nbytes(self):
        return int(nat.lib().psignn_broyden64_bytes(self.handle))

    def solve(self, x0, eps, poll_every=16):
        """From ``x0`` ((N, 10), float32 widened exactly or float64).  Returns ``result`` (the lowest-rel iterate, float64),
        ``lowest``, ``nstep`` (the 1-based step of that iterate), ``n_iter`` (steps taken), ``prot_break``, ``stop_reason``
        (0 threshold, 1 rel < eps, 2 plateau, 3 protective break) and ``rel_trace`` / ``abs_trace`` (entry i: after step i + 1;
        padded to ``threshold + 1`` entries with the lowest values as the reference pads them).  Deterministic; ``poll_every``
        (how often the host looks at the done flag) changes nothing in the result."""
        if self.handle is None or self.fmap.handle is None:
            raise nat.NativeError("DeviceBroyden64 (or its map) is closed")
        fm = self.fmap
        x0c = fm._state(x0, "x0")
        result = torch.empty_like(x0c)
        info = nat.SolveInfo()
        rel = (C.c_double * self.threshold)()
        abs_ = (C.c_double * self.threshold)()
        with torch.cuda.device(self.device):
            nat.check(nat.lib().psignn_broyden64_solve(
                self.handle, nat.ptr(fm.wflat), fm.weights.n_layers, nat.ptr(x0c), nat.ptr(fm.h0), nat.ptr(fm.prb), nat.ptr(fm.nrm),
                float(eps), int(poll_every), nat.ptr(result), C.byref(info), rel, abs_, nat.stream_ptr(self.device)),
                "psignn_broyden64_solve")
        return self._result(info, rel, abs_, result)

    def _result(self, info, rel, abs_, result):
        n_it = int(info.n_iter)
        pad = self.threshold + 1 - n_it
        return {"result": result, "lowest": float(info.lowest), "nstep": int(info.nstep), "n_iter": n_it,
                "prot_break": bool(info.prot_break), "stop_reason": int(info.stop_reason),
                "rel_trace": list(rel[:n_it]) + [float(info.lowest)] * pad,
                "abs_trace": list(abs_[:n_it]) + [float(info.lowest_abs)] * pad}

    def solve_adjoint(self, h_star, grad, eps, poll_every=16):
        """``y = J_f(h*)^T y + grad`` from ``y = 0`` with the recurrences of ``solve`` (``psignn_broyden64_solve_adjoint``): the
        reference's backward hook in double precision, one ``psignn_f64_vjp`` with ``add = grad`` per step.  ``h_star``, ``grad``:
        (N, 10), float32 (widened exactly) or float64.  Returns the dict of ``solve``."""
        if self.handle is None or self.fmap.handle is None:
            raise nat.NativeError("DeviceBroyden64 (or its map) is closed")
        fm = self.fmap
        nat.require_default_width(getattr(getattr(fm, "weights", None), "width", D), "DeviceBroyden64.solve_adjoint")
        hs, gr = fm._states((h_star, "h_star"), (grad, "grad"))
        result = torch.empty_like(gr)
        info = nat.SolveInfo()
        rel = (C.c_double * self.threshold)()
        abs_ = (C.c_double * self.threshold)()
        work, n = fm._work(True)
        with torch.cuda.device(self.device):
            nat.check(nat.lib().psignn_broyden64_solve_adjoint(
                self.handle, nat.ptr(fm.wflat), fm.weights.n_layers, nat.ptr(hs), nat.ptr(fm.h0), nat.ptr(fm.prb), nat.ptr(fm.nrm),
                nat.ptr(gr), float(eps), int(poll_every), nat.ptr(work), n, nat.ptr(result), C.byref(info), rel, abs_,
                nat.stream_ptr(self.device)), "psignn_broyden64_solve_adjoint")
        return self._result(info, rel, abs_, result)


class DeviceGmres64:
    """Restarted GMRES(m) in float64 for the adjoint system ``y = J_f(h*)^T y + grad`` on a ``FixedPointMap64``
    (``psignn_gmres64_*``, csrc/krylov_f64.hip): the float64 adjoint at any size.  The basis is stored in float64,
    ``(m + 1) * N * 10 * 8`` bytes; creation raises ``NativeError`` naming that size when the device cannot hold it."""

    def __init__(self, fmap64, m):
        if getattr(fmap64, "handle", None) is None:
            raise nat.NativeError("DeviceGmres64 needs an open FixedPointMap64")
        self.fmap, self.m, self.device = fmap64, int(m), fmap64.device
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            nat.check(nat.lib().psignn_gmres64_create(C.byref(h), fmap64.handle, self.m), "psignn_gmres64_create")
        self.handle = h
        self._fin = weakref.finalize(self, nat.lib().psignn_gmres64_destroy, h)

    def close(self):
        self._fin()
        self.handle = None

    @property
    def nbytes(self):
        return int(nat.lib().psignn_gmres64_bytes(self.handle))

    def solve_adjoint(self, h_star, grad, eps, max_products, poll_every=8):
        """From ``y = 0``; ``h_star``, ``grad``: (N, 10), float32 (widened exactly) or float64.  Returns the dict of
        ``DeviceGmres.solve_adjoint`` with a float64 ``result``: ``nstep`` = products spent, ``lowest``, ``rel_trace`` /
        ``abs_trace`` with one entry per cycle, ``n_cycles``, ``stop`` (one of ``GMRES_STOPS``), ``n_reorth``.  Deterministic;
        ``poll_every`` changes neither bits nor counts."""
        return self._adjoint(h_star, grad, eps, max_products, poll_every, None)

    def _adjoint(self, h_star, grad, eps, max_products, poll_every, opts):
        """``opts``: None (``psignn_gmres64_solve_adjoint``) or a checked ``nat.Gmres64Opts`` (``..._opts``)."""
        if self.handle is None or self.fmap.handle is None:
            raise nat.NativeError("DeviceGmres64 (or its map) is closed")
        if int(max_products) < 1:
            raise nat.NativeError(f"max_products must be >= 1, got {max_products}")
        fm = self.fmap
        nat.require_default_width(getattr(getattr(fm, "weights", None), "width", D), "DeviceGmres64.solve_adjoint")
        hs, gr = fm._states((h_star, "h_star"), (grad, "grad"))
        result = torch.empty_like(gr)
        info = nat.GmresAdjointInfo() if opts is None else nat.Gmres64Info()
        cap = int(max_products) // 2 + 3
        rel, abs_ = (C.c_double * cap)(), (C.c_double * cap)()
        work, n = fm._work(True)
        lead = (self.handle, nat.ptr(fm.wflat), fm.weights.n_layers, nat.ptr(hs), nat.ptr(fm.h0), nat.ptr(fm.prb), nat.ptr(fm.nrm),
                nat.ptr(gr), float(eps), int(max_products), int(poll_every))
        tail = (nat.ptr(work), n, nat.ptr(result), C.byref(info), rel, abs_, nat.stream_ptr(self.device))
        with torch.cuda.device(self.device):
            if opts is None:
                nat.check(nat.lib().psignn_gmres64_solve_adjoint(*lead, *tail), "psignn_gmres64_solve_adjoint")
            else:
                nat.check(nat.lib().psignn_gmres64_solve_adjoint_opts(*lead, C.byref(opts), *tail), "psignn_gmres64_solve_adjoint_opts")
        return self._dict(info, rel, abs_, result, opts)

    def solve_shifted(self, h, b, shift=1.0, transposed=False, eta=1e-2, max_products=200, poll_every=8):
        """``shift * delta = A delta + b`` from ``delta = 0`` (``psignn_gmres64_solve_shifted``), ``A = J_f(h)`` or, ``transposed``,
        ``J_f(h)^T``: the linear system of a Newton step on ``f(x) - x`` with a pseudo-transient shift, and its dual.  ``shift`` finite
        and >= 1; ``h``, ``b``: (N, 10), float32 (widened exactly) or float64.  Returns the dict of ``solve_adjoint``; ``rel_trace``
        and ``lowest`` are the linear measure ``|A delta + b - shift delta| / |b|``, met at ``rel <= eta``.  ``b = 0`` gives
        ``delta = 0`` without a product.  Deterministic; ``poll_every`` changes neither bits nor counts."""
        return self._shifted(h, b, shift, transposed, eta, max_products, poll_every, None)

    def _shifted(self, h, b, shift, transposed, eta, max_products, poll_every, opts):
        """``opts``: None (``psignn_gmres64_solve_shifted``) or a checked ``nat.Gmres64Opts`` (``..._opts``)."""
        if self.handle is None or self.fmap.handle is None:
            raise nat.NativeError("DeviceGmres64 (or its map) is closed")
        if int(max_products) < 1:
            raise nat.NativeError(f"max_products must be >= 1, got {max_products}")
        if not (math.isfinite(float(shift)) and float(shift) >= 1.0):
            raise nat.NativeError(f"shift must be finite and >= 1, got {shift}")
        if not (math.isfinite(float(eta)) and float(eta) >= 0.0):
            raise nat.NativeError(f"eta must be finite and >= 0, got {eta}")
        fm = self.fmap
        nat.require_default_width(getattr(getattr(fm, "weights", None), "width", D), "DeviceGmres64.solve_shifted")
        hs, bc = fm._states((h, "h"), (b, "b"))
        result = torch.empty_like(bc)
        info = nat.GmresAdjointInfo() if opts is None else nat.Gmres64Info()
        cap = int(max_products) // 2 + 3
        rel, abs_ = (C.c_double * cap)(), (C.c_double * cap)()
        work, n = fm._work_both()
        lead = (self.handle, nat.ptr(fm.wflat), fm.weights.n_layers, nat.ptr(hs), nat.ptr(fm.h0), nat.ptr(fm.prb), nat.ptr(fm.nrm),
                nat.ptr(bc), float(shift), int(bool(transposed)), float(eta), int(max_products), int(poll_every))
        tail = (nat.ptr(work), n, nat.ptr(result), C.byref(info), rel, abs_, nat.stream_ptr(self.device))
        with torch.cuda.device(self.device):
            if opts is None:
                nat.check(nat.lib().psignn_gmres64_solve_shifted(*lead, *tail), "psignn_gmres64_solve_shifted")
            else:
                nat.check(nat.lib().psignn_gmres64_solve_shifted_opts(*lead, C.byref(opts), *tail), "psignn_gmres64_solve_shifted_opts")
        return self._dict(info, rel, abs_, result, opts)

    @staticmethod
    def _dict(info, rel, abs_, result, opts):
        out = DeviceGmres._result(info, rel, abs_, result)
        if opts is not None:
            out["n_aug"], out["augment"] = int(info.n_aug), int(opts.augment)
        return out


AUGMENT_MAX = 8   # psignn_gmres64_create_aug


def gmres64_opts(augment, stall, handle_augment, who, struct=None):
    """The checked ``psignn_gmres64_opts_t`` of one solve: ``augment`` (None: the handle's) in ``0 .. handle_augment``, ``stall`` in
    ``(0, 1]``.  Raises ``NativeError`` before any native call.  ``struct``: another structure of the same two fields
    (``nat.GmresOpts`` of the fp32 solver)."""
    a = int(handle_augment if augment is None else augment)
    if not 0 <= a <= int(handle_augment):
        raise nat.NativeError(f"{who}: augment must be in 0 .. {int(handle_augment)} (the handle's), got {augment}")
    st = float(stall)
    if not 0.0 < st <= 1.0:   # (a NaN is not)
        raise nat.NativeError(f"{who}: stall must be in (0, 1], got {stall}")
    return (nat.Gmres64Opts if struct is None else struct)(a, st)


def check_augment(augment, m, who):
    if not 0 <= int(augment) <= min(int(m) - 1, AUGMENT_MAX):
        raise nat.NativeError(f"{who}: augment must be in 0 .. min(m - 1, {AUGMENT_MAX}) = {min(int(m) - 1, AUGMENT_MAX)}, got {augment}")
    return int(augment)


class DeviceGmres64Aug(DeviceGmres64):
    """``DeviceGmres64`` with augmented restarts (LGMRES) and a settable stall ratio (``psignn_gmres64_create_aug``,
    ``psignn_gmres64_solve_*_opts``; the method: the header of csrc/krylov_f64.hip).  The handle holds a ring of ``augment + 1``
    vectors beside the basis; a solve keeps the ``augment`` newest corrections of its cycles and searches them in the last steps of
    the next cycle.  ``stall``: the solve ends on a cycle with ``not rel <= stall * prev_rel``; 0.5 is ``DeviceGmres64``'s rule, 1.0
    stops only when a cycle does not lower ``rel``.  ``augment=0, stall=0.5`` launches the kernels of ``DeviceGmres64`` and gives its
    bits.  A class of its own because the signatures of ``DeviceGmres64`` are pinned."""

    def __init__(self, fmap64, m, augment=0):
        if getattr(fmap64, "handle", None) is None:
            raise nat.NativeError("DeviceGmres64Aug needs an open FixedPointMap64")
        self.augment = check_augment(augment, m, "DeviceGmres64Aug")
        self.fmap, self.m, self.device = fmap64, int(m), fmap64.device
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            nat.check(nat.lib().psignn_gmres64_create_aug(C.byref(h), fmap64.handle, self.m, self.augment), "psignn_gmres64_create_aug")
        self.handle = h
        self._fin = weakref.finalize(self, nat.lib().psignn_gmres64_destroy, h)

    def solve_adjoint(self, h_star, grad, eps, max_products, poll_every=8, augment=None, stall=0.5):
        """``DeviceGmres64.solve_adjoint`` with ``augment`` (None: the handle's) and ``stall``.  The dict gains ``n_aug`` (the
        augmentation steps of the solve) and ``augment``."""
        opts = gmres64_opts(augment, stall, self.augment, "DeviceGmres64Aug.solve_adjoint")
        return self._adjoint(h_star, grad, eps, max_products, poll_every, opts)

    def solve_shifted(self, h, b, shift=1.0, transposed=False, eta=1e-2, max_products=200, poll_every=8, augment=None, stall=0.5):
        """``DeviceGmres64.solve_shifted`` with ``augment`` (None: the handle's) and ``stall``; the dict gains ``n_aug``, ``augment``."""
        opts = gmres64_opts(augment, stall, self.augment, "DeviceGmres64Aug.solve_shifted")
        return self._shifted(h, b, shift, transposed, eta, max_products, poll_every, opts)


NEWTON_STOPS = ("threshold", "tolerance", "rejects")   # stop_reason of psignn_newton64_info_t


def newton64_policy(sigma, g_old, g_new, growth=2.0, reject_floor=0.0625, sigma_off=1e-8):
    """``psignn_newton64_policy`` (host only, no GPU needed): ``(accepted, next sigma)`` of one attempted step of
    ``DeviceNewton64`` from the shift it ran with and ``|g|`` before and at the trial point."""
    acc = C.c_int(0)
    nxt = nat.lib().psignn_newton64_policy(float(sigma), float(g_old), float(g_new), float(growth), float(reject_floor),
                                           float(sigma_off), C.byref(acc))
    return bool(acc.value), float(nxt)


class DeviceNewton64:
    """Newton-Krylov root-find of ``g(x) = f(x) - x`` in float64 on a ``FixedPointMap64`` with a pseudo-transient shift
    (``psignn_newton64_*``, csrc/newton_f64.hip): attempted step n solves ``(1 + sigma_n) delta = J_f(x_n) delta + g(x_n)`` with
    ``DeviceGmres64.solve_shifted``'s solve (restart length ``m``), evaluates ``f`` at ``x_n + delta`` and lets
    ``psignn_newton64_policy`` accept or reject from ``|g|`` there.  The basis is ``(m + 1) * N * 10 * 8`` bytes, the state six
    vectors more; creation raises ``NativeError`` naming the bytes when the device cannot hold them.

    The defaults of ``solve`` (``sigma0`` 1, ``eta`` 1e-2, ``max_products`` 200, ``growth`` 2, ``reject_floor`` 1/16, ``sigma_off``
    1e-8, ``max_rejects`` 8, ``threshold`` 50, ``m`` 50) are starting values from float64 CPU runs on the stored fixtures.  They are
    not tuned on a GPU."""

    def __init__(self, fmap64, m=50):
        if getattr(fmap64, "handle", None) is None:
            raise nat.NativeError("DeviceNewton64 needs an open FixedPointMap64")
        nat.require_default_width(getattr(getattr(fmap64, "weights", None), "width", D), "DeviceNewton64")
        self.fmap, self.m, self.device = fmap64, int(m), fmap64.device
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            nat.check(nat.lib().psignn_newton64_create(C.byref(h), fmap64.handle, self.m), "psignn_newton64_create")
        self.handle = h
        self._fin = weakref.finalize(self, nat.lib().psignn_newton64_destroy, h)

    def close(self):
        self._fin()
        self.handle = None

    @property
    def nbytes(self):
        return int(nat.lib().psignn_newton64_bytes(self.handle))

    def solve(self, x0, eps=1e-11, threshold=50, sigma0=1.0, eta=1e-2, max_products=200, growth=2.0, reject_floor=0.0625,
              sigma_off=1e-8, max_rejects=8, poll_every=8):
        """From ``x0`` ((N, 10), float32 widened exactly or float64).  Ends on ``rel = |g| / (|f(x)| + 1e-9) < eps`` (Broyden's
        measure), after ``threshold`` attempted steps or after ``max_rejects`` consecutive rejections.  Returns ``result`` (the
        accepted state with the lowest rel, float64, caller's numbering), ``lowest``, ``nstep`` (the accepted step of that state; 0:
        the start), ``n_iter`` (attempted steps), ``n_products``, ``n_feval``, ``rel_trace`` / ``abs_trace`` (the start and every
        accepted state), ``sigma_trace`` (``sigma0`` and the shift after every decision: entry i is the shift of attempted step i),
        ``accepted``, ``trial_abs`` (``|g|`` at every trial point), ``krylov`` (products per attempted step), ``lin_stop`` (the
        linear solve's stop reason per attempted step, one of ``GMRES_STOPS``) and ``stop_reason`` (one of ``NEWTON_STOPS``).
        A rejected step leaves the state untouched bit for bit.  Deterministic; ``poll_every`` changes neither bits nor counts."""
        return self._solve(x0, eps, threshold, sigma0, eta, max_products, growth, reject_floor, sigma_off, max_rejects, poll_every, None)

    def _solve(self, x0, eps, threshold, sigma0, eta, max_products, growth, reject_floor, sigma_off, max_rejects, poll_every, lin_opts):
        """``lin_opts``: None (``psignn_newton64_solve``) or a checked ``nat.Gmres64Opts`` (``psignn_newton64_solve_opts``)."""
        if self.handle is None or self.fmap.handle is None:
            raise nat.NativeError("DeviceNewton64 (or its map) is closed")
        fm = self.fmap
        nat.require_default_width(getattr(getattr(fm, "weights", None), "width", D), "DeviceNewton64.solve")
        for v, name, low in ((eps, "eps", 0.0), (eta, "eta", 0.0), (sigma0, "sigma0", 0.0), (sigma_off, "sigma_off", 0.0)):
            if not (math.isfinite(float(v)) and float(v) >= low):
                raise nat.NativeError(f"{name} must be finite and >= {low:g}, got {v}")
        for v, name in ((growth, "growth"), (reject_floor, "reject_floor")):
            if not (math.isfinite(float(v)) and float(v) > 0.0):
                raise nat.NativeError(f"{name} must be finite and > 0, got {v}")
        for v, name in ((threshold, "threshold"), (max_products, "max_products"), (max_rejects, "max_rejects")):
            if int(v) < 1:
                raise nat.NativeError(f"{name} must be >= 1, got {v}")
        x0c = fm._state(x0, "x0")
        result = torch.empty_like(x0c)
        T = int(threshold)
        opts = nat.Newton64Opts(float(eps), float(sigma0), float(eta), float(growth), float(reject_floor), float(sigma_off), T,
                                int(max_products), int(max_rejects), int(poll_every))
        info = nat.Newton64Info()
        rel, abs_, sig, trial = ((C.c_double * (T + 1))() for _ in range(4))
        acc, kry, lst = ((C.c_int32 * T)() for _ in range(3))
        work, n = fm._work_both()
        lead = (self.handle, nat.ptr(fm.wflat), fm.weights.n_layers, nat.ptr(x0c), nat.ptr(fm.h0), nat.ptr(fm.prb), nat.ptr(fm.nrm),
                C.byref(opts))
        tail = (nat.ptr(work), n, nat.ptr(result), C.byref(info), rel, abs_, sig, trial, acc, kry, lst, nat.stream_ptr(self.device))
        with torch.cuda.device(self.device):
            if lin_opts is None:
                nat.check(nat.lib().psignn_newton64_solve(*lead, *tail), "psignn_newton64_solve")
            else:
                nat.check(nat.lib().psignn_newton64_solve_opts(*lead, C.byref(lin_opts), *tail), "psignn_newton64_solve_opts")
        n_it, n_acc = int(info.n_iter), int(info.n_accepted)
        return {"result": result, "lowest": float(info.lowest), "lowest_abs": float(info.lowest_abs), "nstep": int(info.nstep),
                "n_iter": n_it, "n_products": int(info.n_products), "n_feval": int(info.n_feval),
                "rel_trace": list(rel[:n_acc + 1]), "abs_trace": list(abs_[:n_acc + 1]), "sigma_trace": list(sig[:n_it + 1]),
                "accepted": [bool(a) for a in acc[:n_it]], "trial_abs": list(trial[:n_it]), "krylov": list(kry[:n_it]),
                "lin_stop": [GMRES_STOPS[int(c)] for c in lst[:n_it]], "stop_reason": NEWTON_STOPS[int(info.stop_reason)]}


class DeviceNewton64Aug(DeviceNewton64):
    """``DeviceNewton64`` whose linear solves are ``DeviceGmres64Aug``'s (``psignn_newton64_create_aug``,
    ``psignn_newton64_solve_opts``): every linear solve keeps ``augment`` corrections and ends on ``lin_stall``.  ``augment=0,
    lin_stall=0.5`` gives the bits of ``DeviceNewton64``.  A class of its own because the signatures of ``DeviceNewton64`` are pinned."""

    def __init__(self, fmap64, m=50, augment=0):
        if getattr(fmap64, "handle", None) is None:
            raise nat.NativeError("DeviceNewton64Aug needs an open FixedPointMap64")
        nat.require_default_width(getattr(getattr(fmap64, "weights", None), "width", D), "DeviceNewton64Aug")
        self.augment = check_augment(augment, m, "DeviceNewton64Aug")
        self.fmap, self.m, self.device = fmap64, int(m), fmap64.device
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            nat.check(nat.lib().psignn_newton64_create_aug(C.byref(h), fmap64.handle, self.m, self.augment), "psignn_newton64_create_aug")
        self.handle = h
        self._fin = weakref.finalize(self, nat.lib().psignn_newton64_destroy, h)

    def solve(self, x0, eps=1e-11, threshold=50, sigma0=1.0, eta=1e-2, max_products=200, growth=2.0, reject_floor=0.0625,
              sigma_off=1e-8, max_rejects=8, poll_every=8, lin_stall=0.5):
        """``DeviceNewton64.solve``; every linear solve keeps the handle's ``augment`` corrections and ends on ``lin_stall``."""
        lin = gmres64_opts(None, lin_stall, self.augment, "DeviceNewton64Aug.solve")
        return self._solve(x0, eps, threshold, sigma0, eta, max_products, growth, reject_floor, sigma_off, max_rejects, poll_every, lin)


def fixed_point64(batch, state_dict, eps=1e-11, threshold=1000, poll_every=16, solver="broyden", **solver_kwargs):
    """encoder -> float64 solve -> decoder, all in float64 on the device, for a device batch and a reference state dict (default
    latent width).  ``solver="broyden"`` (the default): ``DeviceBroyden64(threshold)``.  ``solver="newton"``:
    ``DeviceNewton64(m)`` from the encoder's ``h0`` with ``eps``, ``threshold`` (attempted steps at most) and ``poll_every`` as given
    here; ``solver_kwargs`` are ``m`` and the other keywords of ``DeviceNewton64.solve``; with ``augment`` or ``lin_stall`` among
    them the solver is ``DeviceNewton64Aug(m, augment)``.
    Returns the solver's dictionary plus ``h0`` (the encoded start) and ``u`` (the decoded result)."""
    if solver not in ("broyden", "newton"):
        raise nat.NativeError(f"fixed_point64: solver must be 'broyden' or 'newton', got {solver!r}")
    if solver == "broyden" and solver_kwargs:
        raise nat.NativeError(f"fixed_point64: solver 'broyden' takes no further keywords, got {sorted(solver_kwargs)}")
    w = PackedWeights64(state_dict)
    ae = lambda k: state_dict["autoencoder." + k]
    enc = [ae(f"encoder.mlp.mlp.{i}.{p}") for i, p in ((0, "weight"), (0, "bias"), (2, "weight"), (2, "bias"))]
    dec = [ae(f"decoder.mlp.mlp.{i}.{p}") for i, p in ((0, "weight"), (0, "bias"), (2, "weight"), (2, "bias"))]
    plan = plan_for(batch)
    h0 = mlp2_64(batch.x, *enc)
    fmap = FixedPointMap64(plan, w, h0, batch.prb_data, batch.edge_attr, getattr(batch, "unit_normal_vector", None))
    sv = None
    try:
        if solver == "newton":
            kw = dict(solver_kwargs)
            if "augment" in kw or "lin_stall" in kw:
                sv = DeviceNewton64Aug(fmap, kw.pop("m", 50), kw.pop("augment", 0))
            else:
                sv = DeviceNewton64(fmap, kw.pop("m", 50))
            out = sv.solve(h0, eps=eps, threshold=threshold, poll_every=poll_every, **kw)
        else:
            sv = DeviceBroyden64(fmap, threshold)
            out = sv.solve(h0, eps, poll_every)
    finally:
        if sv is not None:
            sv.close()
        fmap.close()
    out["h0"] = h0
    out["u"] = mlp2_64(out["result"], *dec)
    return out


def adjoint64(batch, state_dict, h_star, grad, solver="gmres", eps=1e-11, m=50, max_products=2000, threshold=800):
    """The adjoint of the implicit backward in float64 on the device, ``y = J_f(h*)^T y + grad``, for a device batch and a reference
    state dict (default latent width): the encoder in float64, then ``solver="gmres"`` (``DeviceGmres64(m)``, budget
    ``max_products``) or ``"broyden"`` (``DeviceBroyden64(threshold)``, the reference's own solver).  ``h_star``, ``grad``: (N, 10),
    float32 (widened exactly) or float64.  Returns the solver's dictionary."""
    if solver not in ("gmres", "broyden"):
        raise nat.NativeError(f"adjoint64: solver must be 'gmres' or 'broyden', got {solver!r}")
    nat.require_default_width(width_of(state_dict), "adjoint64")
    n = int(batch.x.shape[0])
    for t, name in ((h_star, "h_star"), (grad, "grad")):
        if tuple(t.shape) != (n, D):
            raise nat.NativeError(f"{name} has shape {tuple(t.shape)}, expected {(n, D)}")
    w = PackedWeights64(state_dict)
    ae = lambda k: state_dict["autoencoder." + k]
    enc = [ae(f"encoder.mlp.mlp.{i}.{p}") for i, p in ((0, "weight"), (0, "bias"), (2, "weight"), (2, "bias"))]
    plan = plan_for(batch)
    h0 = mlp2_64(batch.x, *enc)
    fmap = FixedPointMap64(plan, w, h0, batch.prb_data, batch.edge_attr, getattr(batch, "unit_normal_vector", None))
    sv = None
    try:
        if solver == "gmres":
            sv = DeviceGmres64(fmap, m)
            return sv.solve_adjoint(h_star, grad, eps, max_products)
        sv = DeviceBroyden64(fmap, threshold)
        return sv.solve_adjoint(h_star, grad, eps)
    finally:
        if sv is not None:
            sv.close()
        fmap.close()


def adjoint64_aug(batch, state_dict, h_star, grad, eps=1e-11, m=50, max_products=2000, augment=0, stall=0.5):
    """``adjoint64(solver="gmres")`` on ``DeviceGmres64Aug(m, augment)`` with ``stall``: the dict gains ``n_aug`` and ``augment``.
    (``implicit_grad64(..., y=adjoint64_aug(...)["result"])`` turns it into parameter gradients.)"""
    nat.require_default_width(width_of(state_dict), "adjoint64_aug")
    n = int(batch.x.shape[0])
    for t, name in ((h_star, "h_star"), (grad, "grad")):
        if tuple(t.shape) != (n, D):
            raise nat.NativeError(f"{name} has shape {tuple(t.shape)}, expected {(n, D)}")
    check_augment(augment, m, "adjoint64_aug")
    gmres64_opts(augment, stall, augment, "adjoint64_aug")
    w = PackedWeights64(state_dict)
    ae = lambda k: state_dict["autoencoder." + k]
    enc = [ae(f"encoder.mlp.mlp.{i}.{p}") for i, p in ((0, "weight"), (0, "bias"), (2, "weight"), (2, "bias"))]
    plan = plan_for(batch)
    h0 = mlp2_64(batch.x, *enc)
    fmap = FixedPointMap64(plan, w, h0, batch.prb_data, batch.edge_attr, getattr(batch, "unit_normal_vector", None))
    sv = None
    try:
        sv = DeviceGmres64Aug(fmap, m, augment)
        return sv.solve_adjoint(h_star, grad, eps, max_products, stall=stall)
    finally:
        if sv is not None:
            sv.close()
        fmap.close()


def implicit_grad64(batch, state_dict, h_star, grad, solver="gmres", eps=1e-11, m=50, max_products=2000, threshold=800, y=None):
    """The implicit backward in float64 on the device, for any loss whose cotangent on ``f(h*)`` is ``grad``: the gradient with
    respect to the ``deqdss.f.*`` parameters and the encoder parameters (dirichlet/psignn/model.py:203-225 and 370-392 in double
    precision).  ``adjoint64``'s solve gives ``y`` (``y`` given: no solve, that ``y`` is used), then
    ``FixedPointMap64.param_vjp(h_star, y)``, then ``mlp2_64_backward(batch.x, dH_init, encoder)``.  Returns ``{"grads": {full
    state-dict name: float64 tensor}, "y", "dh" (``J_f(h*)^T y``), "adjoint": the solver's dictionary | None}``."""
    if solver not in ("gmres", "broyden"):
        raise nat.NativeError(f"adjoint64: solver must be 'gmres' or 'broyden', got {solver!r}")
    nat.require_default_width(width_of(state_dict), "implicit_grad64")
    n = int(batch.x.shape[0])
    for t, name in ((h_star, "h_star"), (grad, "grad"), (y, "y")):
        if t is not None and tuple(t.shape) != (n, D):
            raise nat.NativeError(f"{name} has shape {tuple(t.shape)}, expected {(n, D)}")
    adj = None
    if y is None:
        adj = adjoint64(batch, state_dict, h_star, grad, solver=solver, eps=eps, m=m, max_products=max_products, threshold=threshold)
        y = adj["result"]
    w = PackedWeights64(state_dict)
    enc_names = [f"autoencoder.encoder.mlp.mlp.{i}.{p}" for i, p in ((0, "weight"), (0, "bias"), (2, "weight"), (2, "bias"))]
    enc = [state_dict[k] for k in enc_names]
    h0 = mlp2_64(batch.x, *enc)
    fmap = FixedPointMap64(plan_for(batch), w, h0, batch.prb_data, batch.edge_attr, getattr(batch, "unit_normal_vector", None))
    try:
        named, dh, d_init = fmap.param_vjp(h_star, y)
    finally:
        fmap.close()
    grads = {"deqdss.f." + k: t for k, t in named.items()}
    grads.update(zip(enc_names, mlp2_64_backward(batch.x, d_init, *enc[:3], need_gx=False)[1:]))
    return {"grads": grads, "y": y, "dh": dh, "adjoint": adj}


def jac_loss_grad64(batch, state_dict, h_star, probes):
    """The Jacobian regulariser and its gradient in float64 on the device, for a device batch and a reference state dict (default
    latent width): ``jac_loss = sum_i |J_f(h*)^T v_i|^2 / (n N d)`` over the n probes (jac_loss_estimate,
    dirichlet/psignn/model.py:416-435, which draws one ``torch.randn`` probe; n = 1 is its value), and what ``loss.backward()``
    derives from it: per probe ``FixedPointMap64.vjp_backward(h*, v_i, 2 J^T v_i / (n N d))``, summed in the order of the probes.
    ``probes``: a sequence of (N, 10) tensors or one (n, N, 10) tensor, float32 (widened exactly) or float64; ``h_star``: (N, 10).
    Returns ``{"jac_loss": float, "grads": {full state-dict name of every deqdss.f.* tensor: float64 tensor}, "dh": d jac_loss /
    d h* -- what a caller adds to ``grad`` before ``implicit_grad64`` for the gradient of a step with the regulariser -- and "jtv":
    (n, N, 10), the products J^T v_i}``."""
    nat.require_default_width(width_of(state_dict), "jac_loss_grad64")
    n = int(batch.x.shape[0])
    if tuple(h_star.shape) != (n, D):
        raise nat.NativeError(f"h_star has shape {tuple(h_star.shape)}, expected {(n, D)}")
    probes = list(probes)
    if not probes:
        raise nat.NativeError("jac_loss_grad64: at least one probe is needed")
    for i, v in enumerate(probes):
        if tuple(v.shape) != (n, D):
            raise nat.NativeError(f"probe {i} has shape {tuple(v.shape)}, expected {(n, D)}")
    w = PackedWeights64(state_dict)
    enc = [state_dict[f"autoencoder.encoder.mlp.mlp.{i}.{p}"] for i, p in ((0, "weight"), (0, "bias"), (2, "weight"), (2, "bias"))]
    h0 = mlp2_64(batch.x, *enc)
    fmap = FixedPointMap64(plan_for(batch), w, h0, batch.prb_data, batch.edge_attr, getattr(batch, "unit_normal_vector", None))
    scale = 1.0 / (len(probes) * n * D)
    loss, grads, dh, jtvs = 0.0, None, None, []
    try:
        for v in probes:
            jtv = fmap.vjp(h_star, v)
            named, d, again = fmap.vjp_backward(h_star, v, (2.0 * scale) * jtv)
            loss += float((again * again).sum()) * scale
            jtvs.append(again)
            if grads is None:
                grads, dh = named, d
            else:
                for k in grads:
                    grads[k] = grads[k] + named[k]
                dh = dh + d
    finally:
        fmap.close()
    return {"jac_loss": loss, "grads": {"deqdss.f." + k: t for k, t in grads.items()}, "dh": dh, "jtv": torch.stack(jtvs)}


# ---------------------------------------------------------------------------------------------
# the losses of a training step in float64 (csrc/poisson_cg.hip) and the whole step in one call
# ---------------------------------------------------------------------------------------------
def _columns64(plan, a_ij, *named):
    """``a_ij`` ((E,) or (E, 1)) and (N,) or (N, 1) tensors as flat contiguous float64 device tensors; every shape is checked before any
    tensor is touched."""
    for t, name in named:
        if t.numel() != plan.N or t.dim() > 2 or (t.dim() == 2 and t.shape[1] != 1):
            raise nat.NativeError(f"{name} has shape {tuple(t.shape)}, expected {(plan.N, 1)}")
        if plan.N == 0:
            raise nat.NativeError(f"{name} is empty")
    if a_ij.numel() != plan.E:
        raise nat.NativeError(f"a_ij has {a_ij.numel()} values, the plan {plan.E} edges")
    return [_f64c(a_ij, "a_ij").reshape(-1)] + [_f64c(t, name).reshape(-1) for t, name in named]


def residual64(plan, a_ij, u, y):
    """``A u - y`` in float64 (``psignn_residual_f64``), A = COO(edge_index, a_ij) including the diagonal (model.py:157-167):
    (N, 1) float64.  ``a_ij``: the (E,) or (E, 1) values in ``edge_index`` order; ``u``, ``y``: (N,) or (N, 1).  Inputs are float32
    (widened exactly) or float64; the plan's own fp32 copy of ``a_ij`` is not read.  Deterministic."""
    ac, uc, yc = _columns64(plan, a_ij, (u, "u"), (y, "y"))
    out = torch.empty_like(uc)
    with torch.cuda.device(uc.device):
        nat.check(nat.lib().psignn_residual_f64(plan.handle, nat.ptr(ac), nat.ptr(uc), nat.ptr(yc), nat.ptr(out),
                                                nat.stream_ptr(uc.device)), "psignn_residual_f64")
    return out.reshape(-1, 1)


def residual64_t(plan, a_ij, r):
    """``A^T r`` in float64 (``psignn_residual_t_f64``): what autograd sends from the residual to ``u``.  Shapes and dtypes as
    ``residual64``; (N, 1) float64.  Deterministic."""
    ac, rc = _columns64(plan, a_ij, (r, "r"))
    out = torch.empty_like(rc)
    with torch.cuda.device(rc.device):
        nat.check(nat.lib().psignn_residual_t_f64(plan.handle, nat.ptr(ac), nat.ptr(rc), nat.ptr(out), nat.stream_ptr(rc.device)),
                  "psignn_residual_t_f64")
    return out.reshape(-1, 1)


def mse64(a, b=None, need_grad=False):
    """``mean((a - b)^2)`` in float64 (``psignn_mse_f64``; ``b`` None: zeros): (loss as a 0-dim float64 device tensor,
    ``2 (a - b) / a.numel()`` in the shape of ``a`` | None).  Inputs are float32 (widened exactly) or float64.  One partial per
    chunk of ``psignn_mse_f64_chunk()`` elements, added in a fixed order: deterministic."""
    if b is not None and tuple(b.shape) != tuple(a.shape):
        raise nat.NativeError(f"mse64: a has shape {tuple(a.shape)}, b {tuple(b.shape)}")
    n = a.numel()
    if n == 0:
        raise nat.NativeError("mse64: a is empty")
    ac = _f64c(a, "a")
    bc = None if b is None else _f64c(b, "b")
    l = nat.lib()
    nw = int(l.psignn_mse_f64_workspace_doubles(n))
    loss = torch.empty((), dtype=torch.float64, device=ac.device)
    grad = torch.empty_like(ac) if need_grad else None
    work = torch.empty(nw, dtype=torch.float64, device=ac.device)
    with torch.cuda.device(ac.device):
        nat.check(l.psignn_mse_f64(nat.ptr(ac), nat.ptr(bc), n, float(n), nat.ptr(loss), nat.ptr(grad), nat.ptr(work), nw,
                                   nat.stream_ptr(ac.device)), "psignn_mse_f64")
    return loss, grad


def train_step64(batch, state_dict, h_star=None, y=None, jac_weight=0.0, probe=None, fw_eps=1e-11, fw_threshold=1000, solver="gmres",
                 eps=1e-11, m=50, max_products=2000, threshold=800):
    """One training step of ``ModelDEQDSS`` in float64 on the device, for a device batch and a reference state dict (default latent
    width): the losses of ``_train_forward`` (model.py:58-99) and what ``loss.backward()`` leaves in every parameter for
    ``loss = residual_loss + jac_weight * jacobian_loss + encoder_loss + autoencoder_loss`` (training_class.py:155-159).

    ``h_star`` given: the state the step is taken at; otherwise ``fixed_point64(fw_eps, fw_threshold)``.  ``y`` given: the adjoint
    ``y = J^T y + grad_h`` is taken as solved by it; otherwise ``adjoint64(solver, eps, m, max_products, threshold)``.  ``probe``:
    the (N, 10) probe of the Jacobian regulariser, for which the reference draws ``torch.randn``; H* is a leaf of it (model.py:204), so it
    adds nothing to ``grad_h``.  ``jac_weight != 0`` needs a probe; a probe with ``jac_weight == 0`` still reports
    ``jacobian_loss``.

    The chain: ``new_H = f(h*)``, ``u = dec(new_H)``, ``r = A u - y_rhs`` and ``mean(r^2)`` (``residual64`` / ``mse64``), its
    cotangent back through ``residual64_t`` and ``mlp2_64_backward`` to ``grad_h``; the encoder and autoencoder losses at constant
    ``u`` / ``new_H``; ``implicit_grad64`` for f and the encoder; the composition of ``jac_loss_grad64`` for the regulariser, which reaches f's
    parameters and, in a multi-layer dirichlet block, the encoder through ``H_init`` (``FixedPointMap64.vjp_backward_init``).

    Returns ``loss`` (float), ``loss_dic`` (the six keys of ``_train_forward`` as floats; ``mse_loss`` is nan without ``batch.sol``),
    ``grads`` (every name of the state dict -> float64 tensor, exact zeros where autograd leaves none), ``h_star``, ``new_h``,
    ``u``, ``grad_h`` (the cotangent the backward hook receives), ``y``, ``forward`` / ``adjoint`` (the solvers' dictionaries, None
    where the state was given)."""
    nat.require_default_width(width_of(state_dict), "train_step64")
    if solver not in ("gmres", "broyden"):
        raise nat.NativeError(f"train_step64: solver must be 'gmres' or 'broyden', got {solver!r}")
    jac_weight = float(jac_weight)
    if jac_weight != 0.0 and probe is None:
        raise nat.NativeError("train_step64: jac_weight != 0 needs a probe (the reference draws it with randn; a truth needs it handed in)")
    n = int(batch.x.shape[0])
    for t, name in ((h_star, "h_star"), (y, "y"), (probe, "probe")):
        if t is not None and tuple(t.shape) != (n, D):
            raise nat.NativeError(f"{name} has shape {tuple(t.shape)}, expected {(n, D)}")
    ae = lambda which: [f"autoencoder.{which}.mlp.mlp.{i}.{p}" for i, p in ((0, "weight"), (0, "bias"), (2, "weight"), (2, "bias"))]
    enc_names, dec_names = ae("encoder"), ae("decoder")
    enc, dec = [state_dict[k] for k in enc_names], [state_dict[k] for k in dec_names]
    fw = None
    if h_star is None:
        fw = fixed_point64(batch, state_dict, eps=fw_eps, threshold=fw_threshold)
        h_star = fw["result"]
    h_star = _f64c(h_star, "h_star")
    plan = plan_for(batch)
    h0 = mlp2_64(batch.x, *enc)
    fmap = FixedPointMap64(plan, PackedWeights64(state_dict), h0, batch.prb_data, batch.edge_attr, getattr(batch, "unit_normal_vector", None))
    try:
        new_h = fmap(h_star)
    finally:
        fmap.close()
    u = mlp2_64(new_h, *dec)
    # residual term: down to the cotangent of new_H
    res_loss, g_r = mse64(residual64(plan, batch.a_ij, u, batch.y), None, need_grad=True)
    g_u = residual64_t(plan, batch.a_ij, g_r)
    grad_h, *dec_g1 = mlp2_64_backward(new_h, g_u, *dec[:3])
    # encoder and autoencoder terms, u and new_H (then e and u) held constant
    e = mlp2_64(u, *enc)
    enc_loss, g_e = mse64(e, new_h, need_grad=True)
    enc_g2 = mlp2_64_backward(u, g_e, *enc[:3], need_gx=False)[1:]
    back = mlp2_64(e, *dec)
    ae_loss, g_d = mse64(back, u, need_grad=True)
    dec_g2 = mlp2_64_backward(e, g_d, *dec[:3], need_gx=False)[1:]
    # the implicit backward: f's parameters and, through dH_init, the encoder
    imp = implicit_grad64(batch, state_dict, h_star, grad_h, solver=solver, eps=eps, m=m, max_products=max_products, threshold=threshold,
                          y=y)
    grads = dict(imp["grads"])
    jac_loss = 0.0
    if probe is not None:
        # jac_loss_grad64 with one probe, and d psi / dH_init besides.  d psi / dH* goes nowhere: H* is a leaf of the regulariser
        # (model.py:204).  H_init is not: a multi-layer dirichlet block evaluates its Jacobian at states that carry H_init's
        # Dirichlet rows, so there the regulariser reaches the encoder as well; for every other block that cotangent is exact zeros.
        scale = 1.0 / (n * D)
        fmap = FixedPointMap64(plan, PackedWeights64(state_dict), h0, batch.prb_data, batch.edge_attr, getattr(batch, "unit_normal_vector", None))
        try:
            named, _, jtv, d_init = fmap.vjp_backward_init(h_star, probe, (2.0 * scale) * fmap.vjp(h_star, probe))
        finally:
            fmap.close()
        jac_loss = float((jtv * jtv).sum()) * scale
        if jac_weight != 0.0:
            for k, t in named.items():
                grads["deqdss.f." + k] = grads["deqdss.f." + k] + jac_weight * t
            if n_layers_of(state_dict) > 1 and not is_mixed_state_dict(state_dict):
                for k, t in zip(enc_names, mlp2_64_backward(batch.x, d_init, *enc[:3], need_gx=False)[1:]):
                    grads[k] = grads[k] + jac_weight * t
    for k, t in zip(enc_names, enc_g2):
        grads[k] = grads[k] + t
    for k, a, b in zip(dec_names, dec_g1, dec_g2):
        grads[k] = a + b
    for k, t in state_dict.items():
        if k not in grads:
            grads[k] = torch.zeros(tuple(t.shape), dtype=torch.float64, device=u.device)
        else:
            grads[k] = grads[k].reshape(tuple(t.shape))
    sol = getattr(batch, "sol", None)
    idx = torch.where(batch.tags == 1)[0]   # model.py:87 (mixed: one-hot tags -> every row)
    loss_dic = {"residual_loss": float(res_loss), "encoder_loss": float(enc_loss), "autoencoder_loss": float(ae_loss),
                "mse_loss": float("nan") if sol is None else float(mse64(u, sol)[0]),
                "mse_dirichlet": float(mse64(u[idx], batch.x[idx])[0]) if idx.numel() else float("nan"),
                "jacobian_loss": float(jac_loss)}
    loss = loss_dic["residual_loss"] + jac_weight * loss_dic["jacobian_loss"] + loss_dic["encoder_loss"] + loss_dic["autoencoder_loss"]
    return {"loss": loss, "loss_dic": loss_dic, "grads": {k: grads[k] for k in state_dict}, "h_star": h_star, "new_h": new_h, "u": u,
            "grad_h": grad_h, "y": imp["y"], "forward": fw, "adjoint": imp["adjoint"]}
