"""PSI-GNN inference models with the reference's constructor, ``forward()`` and ``state_dict`` layout.

Drop-in for ``tests/model_psignn.py`` (``ModelPSIGNN``, ``ModelPSIGNNIterative``),
``dirichlet/psignn/model.py`` (``ModelDEQDSS``: ``forward`` diagnostics / ``inference`` /
``iterative_inference``) and their mixed (Dirichlet + Neumann) counterparts
``mixed/psignn/test/model_test.py`` / ``mixed/psignn/model.py``.

* ``Model(config)`` takes the reference's config dict (``latent_dim, n_layers, solver, fw_tol, fw_thres,
  bw_tol, bw_thres, path_logs``; ``hidden_dim`` ignored as in the reference).  An optional key
  ``"bc"`` = ``"dirichlet"`` | ``"mixed"`` selects the family (the reference uses two copies of the file).  An optional
  key ``"bw_linearize"`` (default False): the implicit backward, the power method and the Jacobian estimate linearise f
  once at H* and apply the transposed stored linearisation (``engine.Linearization.vjp_p``) where the plan allows it.  On the
  mixed family it gains nothing by itself: its transposed product is the tiled VJP at the state the build kept, so the key only adds
  one build per call there -- unless the optional key ``"lin_neumann"`` is ``"stored"`` (default ``"direct"``; ignored for the
  dirichlet family): every Linearization the model creates (implicit backward, power method, Jacobian estimate, the Newton-Krylov
  route of ``utilities.solver``) then stores the Neumann rows too, and its products are the stored operator and its exact transpose
  on every tile (``engine.Linearization(fmap, neumann="stored")``).  An optional key ``"broyden_history_dtype"`` (default ``torch.float32``; ``torch.bfloat16`` allowed): the
  element type of the stored Broyden pairs of the forward and the adjoint solve (``utilities.solver.broyden(...,
  history_dtype=...)``); it applies when the configured solver is ``utilities.solver.broyden`` and has no effect with any other.
  An optional key ``"jac_backward"`` = ``"gather"`` (default) | ``"tiled"``: the backward of the Jacobian regulariser
  (``_JacLossFn``) on the tile kernels (``FixedPointMap.vjp_backward(..., tiled=True)``) where the map has that form -- tiled plan,
  dirichlet family, single-layer block -- and on the gather kernels everywhere else; any other value raises ``ValueError``.
  An optional key ``"bw_solver"`` = ``None`` (default: the implicit backward runs ``config["solver"]`` like the reference) |
  ``"gmres"``: the backward's linear system y = J^T y + grad is solved by restarted GMRES on the device
  (``engine.DeviceGmres.solve_adjoint``; restart length ``"bw_gmres_m"``, an int in 2..``bw_thres``, default 50 or ``bw_thres`` if that is less) with ``bw_tol`` as
  its tolerance and ``bw_thres`` as its budget of transposed products; with ``bw_linearize`` on the stored linearisation where the plan
  has one, on the VJP kernels otherwise.  A departure from the reference's algorithm, hence opt-in; any other value raises
  ``NativeError``.  The forward solve, ``power_method`` and ``jac_loss_estimate`` are untouched by it.
  An optional key ``"bw_gmres_lockstep"`` (bool, default False; True needs ``bw_solver = "gmres"``, ``NativeError`` naming both keys
  otherwise): the replicas of a list call take the lockstep route with the GMRES adjoint solve -- forward solves through
  ``engine.broyden_solve_batch``, the R adjoint systems through ``engine.gmres_solve_adjoint_batch`` -- where
  ``DeepEquilibrium.lockstep_applies`` says yes; without it replicas with ``bw_solver = "gmres"`` are solved one after the other.
  Two optional keys ``"bw_gmres_augment"`` (int in 0..min(``bw_gmres_m`` - 1, 8), default 0) and ``"bw_gmres_stall"`` (float in
  (0, 1], default 0.5), both needing ``bw_solver = "gmres"`` (``NativeError`` naming the keys otherwise): the GMRES adjoint solve keeps
  that many corrections between restart cycles (LGMRES) and ends on a cycle with ``not rel <= stall * prev_rel``
  (``engine.DeviceGmresAug.solve_adjoint``); with both at their defaults the objects, launches and bits are those without the keys.
  With a non-default value ``last_backward`` carries ``n_aug``, and the replicas of a list call are solved one after the other whatever
  ``bw_gmres_lockstep`` says (``DeepEquilibrium.lockstep_applies`` says no: the lockstep GMRES takes no options).
  An optional key ``"fp_lockstep"`` (bool, default False; True needs ``solver`` = ``utilities.solver.anderson`` or
  ``forward_iteration``, ``NativeError`` naming both keys otherwise): the forward solves of a shard -- ``batch.solve_shard_batched``,
  the replicas of a list call -- run in one lockstep Anderson / Picard solve (``utilities.solver.anderson_batch`` /
  ``forward_iteration_batch``) where ``DeepEquilibrium.fp_lockstep_applies`` says yes (tiled plans of one family, single-layer block,
  more than one mesh); the backward is untouched, and without the key every mesh is solved on its own as before.
* ``load_state_dict(ckpt["state_dict"])`` of a reference checkpoint works unchanged: parameter names
  and shapes are identical.
* ``batch`` is any object with the PyG ``Data`` attributes (see ``data/meshdata.py``), already on the GPU.
* ``ModelDEQDSS.forward`` also takes a list / tuple of batches: the R replicas of the reference's ``DataParallel`` call
  (``dirichlet/psignn/main.py:106``), R independent fixed-point problems solved in lockstep
  (``DeepEquilibrium.train_forward_replicas``; ``loader.DataParallel(net, replicas=R)`` builds the list), every ``loss_dic`` value
  of shape ``(R,)``.  A single batch behaves as it always did.

The numerical work — encoder/decoder MLPs, the GNN block f, the Broyden root-find, the residual
SpMV — runs in libpsignn_hip.so.  No torch_geometric / torch_sparse.
"""
from __future__ import annotations

import os

import torch
import torch.nn as nn

from . import _native as nat
from . import engine
from .utilities import solver as _solver

# ----------------------------------------------------------------------------------------------
# parameter containers (names = the reference's module tree; arithmetic is NOT done by these)
# ----------------------------------------------------------------------------------------------


def initialize_weights_xavier(m, gain=1.0):  # model.py:310-314
    if isinstance(m, nn.Linear):
        nn.init.xavier_uniform_(m.weight, gain=gain)
        if m.bias is not None:
            nn.init.constant_(m.bias, 0)


class MLP(nn.Module):
    """Linear, ReLU, Linear (model.py:316-332).  Two-layer only, like every instance in the reference."""

    def __init__(self, hidden_channels=None, activation=None):
        super().__init__()
        if len(hidden_channels) != 3:
            raise nat.NativeError("the HIP path implements the reference's two-layer MLPs only")
        a, b, c = hidden_channels
        self.mlp = nn.Sequential(nn.Linear(a, b), nn.ReLU(), nn.Linear(b, c)).apply(initialize_weights_xavier)

    def forward(self, x):
        l0, l2 = self.mlp[0], self.mlp[2]
        return engine.mlp2_autograd(x, l0.weight, l0.bias, l2.weight, l2.bias)


class _Phi(nn.Module):
    """Parameter holder of ``Phi_to`` / ``Phi_from`` (model.py:334-368)."""

    def __init__(self, hidden_channels=None, activation=None):
        super().__init__()
        self.mlp = MLP(hidden_channels, activation)


class Phi_to(_Phi):
    pass


class Phi_from(_Phi):
    pass


class Encoder(nn.Module):
    def __init__(self, hidden_channels=None, activation=None):
        super().__init__()
        self.mlp = MLP(hidden_channels, activation)

    def forward(self, x):
        return self.mlp(x)


class Decoder(Encoder):
    pass


class Autoencoder(nn.Module):  # model.py:394-406
    def __init__(self, hidden_channels=None, activation=None):
        super().__init__()
        self.encoder = Encoder(hidden_channels, activation)
        self.decoder = Decoder(list(reversed(hidden_channels)), activation)

    def forward(self, x, sens):
        if sens == "latent":
            return self.encoder(self.decoder(x))
        if sens == "physics":
            return self.decoder(self.encoder(x))
        print("Specify autoencoder direction")


class Function(nn.Module):
    """The GNN block f_theta (dirichlet: model.py:263-300; mixed: mixed/psignn/model.py:196-245)."""

    def __init__(self, n_layers=None, latent_dim=None, edge_features_dim=None, second_member_dim=None,
                 activation=None, mixed=False):
        super().__init__()
        if edge_features_dim != 3:
            raise nat.NativeError("HIP kernels are built for edge_features_dim=3")
        # latent_dim: engine.SUPPORTED_WIDTHS.  engine.D has every path; the other widths forward inference only
        self.latent_dim = nat.check_width(latent_dim)
        self.n_layers, self.mixed = n_layers, mixed
        d, p = latent_dim, second_member_dim
        self.laynorm = nn.LayerNorm(d)
        self.phi_to_list = nn.ModuleList([Phi_to([2 * d + 3, d, d], activation) for _ in range(n_layers)])
        self.phi_from_list = nn.ModuleList([Phi_from([2 * d + 3, d, d], activation) for _ in range(n_layers)])
        self.alpha = nn.Sequential(nn.Linear(3 * d + p, 1), nn.Sigmoid()).apply(initialize_weights_xavier)
        self.update_list = nn.ModuleList([MLP([3 * d + p, d, d], activation) for _ in range(n_layers)])
        if mixed:
            self.phi_neumann = Phi_from([2 * d + 3, d, d], activation)
            self.update_neumann = MLP([2 * d + p + 2, d, d], activation)
        self._packed = None
        self._packed_key = None

    def packed(self, device) -> engine.PackedWeights:
        key = (str(device),) + tuple((p.data_ptr(), p._version) for p in self.parameters())
        if self._packed_key != key:
            sd = {"deqdss.f." + k: v for k, v in self.state_dict().items()}
            self._packed = engine.PackedWeights(sd, device)
            self._packed_key = key
        return self._packed

    def bind(self, h_initial, batch) -> engine.FixedPointMap:
        """The map H -> f(H, h_initial, batch) as a device object the solvers understand."""
        plan = engine.plan_for(batch)
        nrm = getattr(batch, "unit_normal_vector", None) if self.mixed else None
        fmap = engine.FixedPointMap(plan, self.packed(h_initial.device), h_initial, batch.prb_data, nrm)
        fmap.lin_neumann = self.lin_neumann
        fmap.jac_backward = self.jac_backward
        return fmap

    lin_neumann = "direct"   # the model's ``lin_neumann`` config value: what the maps bound here give a new Linearization
    jac_backward = "gather"  # the model's ``jac_backward`` config value: the route ``_JacLossFn.backward`` takes on these maps

    def forward(self, h, h_initial, batch):
        return self.bind(h_initial, batch)(h)


class _DEQFn(torch.autograd.Function):
    """new_H = f(H*) with H* = solver(f, H_init), differentiable the way the reference's training variant is
    (dirichlet/psignn/model.py:184-225): the forward solve runs without a graph; backward replaces the incoming
    gradient by the solution y of  y = J_f(H*)^T y + grad  (the reference's ``backward_hook``) and pushes y through
    one application of f: parameter gradients from the HIP parameter-VJP kernels, and for ``H_init`` the Dirichlet
    rows of the cotangent on every layer's output (those rows are copies of ``H_init`` after each layer, model.py:298)."""

    @staticmethod
    def forward(ctx, H_init, deq, batch, names, *params):
        cfg = deq.config_deq
        H0 = H_init.detach()
        fmap = deq.f.bind(H0, batch)
        if cfg["solver"] is _solver.broyden:   # forward solver state kept between training steps on the same plan
            hdt = deq.history_dtype()
            old = getattr(deq, "_fw_key", None)
            if old is None or old[0] is not fmap.plan or old[1] != cfg["fw_thres"] or old[2] != hdt:
                if getattr(deq, "_fw_solver", None) is not None:
                    deq._fw_solver.close()
                deq._fw_solver = engine.DeviceBroyden(plan=fmap.plan, threshold=cfg["fw_thres"], keep_trace=False, history_dtype=hdt,
                                                      width=fmap.width)
                deq._fw_key = (fmap.plan, cfg["fw_thres"], hdt)
            out_fw = _solver.broyden(fmap, H0, threshold=cfg["fw_thres"], eps=cfg["fw_tol"], keep_trace=False,
                                     solver_obj=deq._fw_solver, history_dtype=hdt)
        elif getattr(deq, "presolved", None) is not None:   # a replica slot whose forward solve ran in lockstep with the others'
            out_fw, deq.presolved = deq.presolved, None
        else:
            out_fw = cfg["solver"](fmap, H0, threshold=cfg["fw_thres"], eps=cfg["fw_tol"])
        H_star = out_fw["result"]
        deq.last_forward = out_fw
        _log(deq.path_logs, "forward_iteration.csv", "\n{} \t {}".format(out_fw["lowest"], out_fw["nstep"]))
        ctx.deq, ctx.batch, ctx.names, ctx.fmap = deq, batch, names, fmap
        ctx.save_for_backward(H_star, H0)
        return fmap(H_star)

    @staticmethod
    def backward(ctx, grad):
        H_star, H0 = ctx.saved_tensors
        deq = ctx.deq
        out_bw = deq.implicit_backward(H_star, H0, ctx.batch, grad.contiguous())
        deq.last_backward = out_bw
        _log(deq.path_logs, "backward_iteration.csv", "\n{} \t {}".format(out_bw["lowest"], out_bw["nstep"]))
        y = out_bw["result"]
        # g_init: the Dirichlet rows of the cotangent on every layer's output (f copies them from H_init after each layer)
        grads, _, g_init = ctx.fmap.param_vjp_init(H_star, y)
        return (g_init, None, None, None) + tuple(grads[n] for n in ctx.names)


class _ReplicaSlot:
    """What one replica slot of ``DeepEquilibrium.train_forward_replicas`` keeps between training steps: its forward and
    adjoint solver (``_fw_solver`` / ``_bw_solver``) and its linearisation handle (``_bw_lin``), keyed and replaced like the
    single-batch ones of ``DeepEquilibrium``, whose solver-side methods it borrows (so that the sequential fallback is the
    existing single-mesh route, one slot after the other)."""

    def __init__(self, deq, index):
        self.f, self.config_deq, self.path_logs = deq.f, deq.config_deq, deq.path_logs
        self.index, self.sink = index, None
        self._last_backward = None

    @property
    def last_backward(self):
        return self._last_backward

    @last_backward.setter
    def last_backward(self, out):
        self._last_backward = out
        if self.sink is not None:   # the model's per-replica list of this step
            self.sink[self.index] = out

    def solver(self, which, plan, threshold, hdt, shard_elems):
        """The slot's ``which`` = "fw" | "bw" solver for (plan, threshold, history dtype, shard size); closed and remade when
        the key changes."""
        key = (plan, threshold, hdt, shard_elems)
        old = getattr(self, f"_{which}_key", None)
        if old is None or old[0] is not plan or old[1:] != key[1:]:
            sv = getattr(self, f"_{which}_solver", None)
            if sv is not None:
                sv.close()
            setattr(self, f"_{which}_solver", engine.DeviceBroyden(plan=plan, threshold=threshold, keep_trace=False,
                                                                  shard_elems=shard_elems, history_dtype=hdt))
            setattr(self, f"_{which}_key", key)
        return getattr(self, f"_{which}_solver")

    def gmres(self, plan, m, shard_elems):
        """The slot's GMRES handle for (plan, restart length, shard size), keyed and replaced like ``solver()``.  It shares the
        attribute of the single-batch route's handle (``implicit_backward``), whose key has no shard size: either route remakes
        the handle the other left."""
        key = (plan, m, shard_elems)
        old = getattr(self, "_bw_gmres_key", None)
        if old is None or len(old) != 3 or old[0] is not plan or old[1:] != key[1:]:
            if getattr(self, "_bw_gmres", None) is not None:
                self._bw_gmres.close()
            self._bw_gmres = engine.DeviceGmres(plan.N * engine.D, plan.device, m, shard_elems=shard_elems)
            self._bw_gmres_key = key
        return self._bw_gmres

    def close(self):
        for name in ("_fw_solver", "_bw_solver", "_bw_lin", "_bw_gmres"):
            obj = getattr(self, name, None)
            if obj is not None:
                obj.close()
                setattr(self, name, None)
        self._fw_key = self._bw_key = self._bw_gmres_key = None


class _DEQReplicasFn(torch.autograd.Function):
    """``_DEQFn`` over R replicas at once (the reference's ``DataParallel`` replicas, dirichlet/psignn/main.py:106, each with
    the backward hook of model.py:210-223): the R forward solves run in lockstep (``engine.broyden_solve_batch``); backward
    builds R linearisations, each at its H*, and solves the R adjoint fixed points in lockstep
    (``engine.broyden_solve_adjoint_batch``; with ``bw_solver = "gmres"`` and ``bw_gmres_lockstep`` the R restarted GMRES solves,
    ``engine.gmres_solve_adjoint_batch`` on each slot's GMRES handle), then pushes each y_r through one application of f and adds
    the parameter gradients up in replica order.  Where ``engine.shard_batchable`` / ``engine.adjoint_batchable`` /
    ``engine.gmres_adjoint_batchable`` say no, the same solver objects run one mesh after the other."""

    @staticmethod
    def forward(ctx, deq, batches, names, *tensors):
        R = len(batches)
        cfg = deq.config_deq
        H0s = [t.detach() for t in tensors[:R]]
        fmaps = [deq.f.bind(h, b) for h, b in zip(H0s, batches)]
        slots = deq._replica_slots(R)
        shard = sum(f.plan.N for f in fmaps) * engine.D
        solvers = [sl.solver("fw", f.plan, cfg["fw_thres"], torch.float32, shard) for sl, f in zip(slots, fmaps)]
        if engine.shard_batchable(solvers):
            outs = engine.broyden_solve_batch(solvers, fmaps, cfg["fw_tol"])
        else:
            outs = [sv.solve(f, cfg["fw_tol"]) for sv, f in zip(solvers, fmaps)]
        for o in outs:
            o.update(eps=cfg["fw_tol"], threshold=cfg["fw_thres"])
            _log(deq.path_logs, "forward_iteration.csv", "\n{} \t {}".format(o["lowest"], o["nstep"]))
        deq.last_forward = outs
        ctx.deq, ctx.fmaps, ctx.names, ctx.slots, ctx.shard = deq, fmaps, names, slots, shard
        H_stars = [o["result"] for o in outs]
        ctx.save_for_backward(*H_stars)
        return tuple(f(h) for f, h in zip(fmaps, H_stars))

    @staticmethod
    def backward(ctx, *grads):
        deq, fmaps, slots = ctx.deq, ctx.fmaps, ctx.slots
        cfg = deq.config_deq
        H_stars = ctx.saved_tensors
        gs = [torch.zeros_like(h) if g is None else g.contiguous() for g, h in zip(grads, H_stars)]
        lins = [sl._linearization(f, h) for sl, f, h in zip(slots, fmaps, H_stars)]
        if cfg.get("bw_gmres_lockstep"):   # (with bw_solver = "gmres": checked when the model was made)
            m = int(cfg.get("bw_gmres_m", 50))
            solvers = [sl.gmres(f.plan, m, ctx.shard) for sl, f in zip(slots, fmaps)]
            if engine.gmres_adjoint_batchable(solvers, lins):
                outs = engine.gmres_solve_adjoint_batch(solvers, lins, gs, cfg["bw_tol"], cfg["bw_thres"])
            else:
                outs = [sv.solve_adjoint(f, h, g, cfg["bw_tol"], cfg["bw_thres"], lin=l)
                        for sv, f, h, g, l in zip(solvers, fmaps, H_stars, gs, lins)]
        else:
            solvers = [sl.solver("bw", f.plan, cfg["bw_thres"], torch.float32, ctx.shard) for sl, f in zip(slots, fmaps)]
            if engine.adjoint_batchable(solvers, lins):
                outs = engine.broyden_solve_adjoint_batch(solvers, lins, gs, cfg["bw_tol"])
            else:
                outs = [sv.solve_adjoint(f, h, g, cfg["bw_tol"], lin=l) for sv, f, h, g, l in zip(solvers, fmaps, H_stars, gs, lins)]
        total, g_inits = None, []
        for r, (o, f, h) in enumerate(zip(outs, fmaps, H_stars)):
            o.update(eps=cfg["bw_tol"], threshold=cfg["bw_thres"])
            deq.last_backward[r] = o
            _log(deq.path_logs, "backward_iteration.csv", "\n{} \t {}".format(o["lowest"], o["nstep"]))
            pg, _, g_init = f.param_vjp_init(h, o["result"])
            g_inits.append(g_init)
            total = pg if total is None else {n: total[n] + pg[n] for n in ctx.names}
        return (None, None, None) + tuple(g_inits) + tuple(total[n] for n in ctx.names)


class _JacLossFn(torch.autograd.Function):
    """jac_loss = |v^T J_f(H*)|^2 / (N d) with its gradient w.r.t. the parameters of f: the reference builds the VJP with
    ``create_graph=True`` (jac_loss_estimate, dirichlet/psignn/model.py:416-435) and lets ``loss.backward()`` run the
    double backward; here backward is the HIP backward-of-the-VJP (csrc/gather_backward.hip; with the config key
    ``jac_backward = "tiled"`` its tile form, csrc/fgnn_tile_jr.hip, where the map has one).  H* is a leaf in the
    reference (model.py:204), so nothing flows back into the solve."""

    @staticmethod
    def forward(ctx, fmap, H_star, v, names, *params):
        g = fmap.vjp(H_star, v)
        ctx.fmap, ctx.names = fmap, names
        ctx.save_for_backward(H_star, v, g)
        return g.norm() ** 2 / H_star.numel()

    @staticmethod
    def backward(ctx, grad_out):
        H_star, v, g = ctx.saved_tensors
        # "tiled": the tile kernels where the map has that form; the gather kernels otherwise (untiled plan, mixed family, n_layers > 1)
        tiled = ctx.fmap.jac_backward == "tiled" and ctx.fmap.can_tile_vjp_backward()
        grads, _ = ctx.fmap.vjp_backward(H_star, v, g * (2.0 * grad_out / H_star.numel()), tiled=tiled)
        return (None, None, None, None) + tuple(grads[n] for n in ctx.names)


def _log(path_logs, name, line):
    if path_logs:
        with open(os.path.join(path_logs, name), "a") as f:
            f.write(line)


class DeepEquilibrium(nn.Module):
    """Inference variant (tests/model_psignn.py:216-243): one solver call, returns the solver dict; plus the
    training variant's differentiable forward (dirichlet/psignn/model.py:184-243) as ``train_forward``."""

    def __init__(self, function=None, config_deq=None):
        super().__init__()
        self.f = function
        self.config_deq = config_deq
        self.path_logs = self.config_deq.get("path_logs")

    def history_dtype(self):
        """Element type of the stored Broyden pairs (config key ``broyden_history_dtype``, default ``torch.float32``)."""
        return self.config_deq.get("broyden_history_dtype", torch.float32)

    def _solver_kwargs(self):
        # broyden_history_dtype reaches utilities.solver.broyden only; other solvers take the reference's arguments as they are
        if self.config_deq["solver"] is _solver.broyden and self.history_dtype() != torch.float32:
            return {"history_dtype": self.history_dtype()}
        return {}

    def forward(self, H_init, batch):
        return self.config_deq["solver"](self.f.bind(H_init, batch), H_init,
                                         threshold=self.config_deq["fw_thres"], eps=self.config_deq["fw_tol"],
                                         **self._solver_kwargs())

    inference = forward  # dirichlet/psignn/model.py:245-253

    def train_forward(self, H_init, batch, generator=None):
        """(new_H_star, jacobian_loss) of the training variant.  With gradients enabled new_H_star carries the
        implicit-function backward; without (validation) the spectral radius is logged like the reference does.
        The Jacobian regulariser carries its gradient w.r.t. the parameters of f (``_JacLossFn``; the reference's launch
        scripts train with ``jac_weight 1.0``)."""
        if torch.is_grad_enabled():
            nat.require_default_width(self.f.latent_dim, "training (the implicit backward)")
            named = list(self.f.named_parameters())
            new_H = _DEQFn.apply(H_init, self, batch, tuple(n for n, _ in named), *[p for _, p in named])
            H_star = self.last_forward["result"]
        else:
            out_fw = self.forward(H_init, batch)
            self.last_forward = out_fw
            H_star = out_fw["result"]
            new_H = self.f.bind(H_init, batch)(H_star)
        if torch.is_grad_enabled():
            # differentiable w.r.t. the parameters of f, as in the reference (vecs = 1, model.py:207)
            v = torch.randn(H_star.shape, device=H_star.device, generator=generator)
            self.last_probe = v
            jac_loss = _JacLossFn.apply(self.f.bind(H_init.detach(), batch), H_star, v, tuple(n for n, _ in named),
                                        *[p for _, p in named])
            return new_H, jac_loss
        with torch.no_grad():
            # both diagnostics at the same H*: one linearisation for the two of them
            shared = (self._linearization(self.f.bind(H_init.detach(), batch), H_star)
                      if self.path_logs and self._linearize_default(None) else None)
            jac_loss = self.jac_loss_estimate(H_star, H_init.detach(), batch, vecs=1, generator=generator, linearize=shared)
            if not torch.is_grad_enabled() and self.path_logs:
                _, sradius = self.power_method(H_star, H_init.detach(), batch, n_iters=150, generator=generator,
                                               linearize=shared)
                _log(self.path_logs, "spectral_radius.csv", "\n{}".format(sradius.item()))
        return new_H, jac_loss

    # ---- R replicas in one step (the reference's DataParallel call with num_gpus = R, dirichlet/psignn/main.py:106)
    def _replica_slots(self, R):
        slots = self.__dict__.setdefault("_slots", [])
        while len(slots) < R:
            slots.append(_ReplicaSlot(self, len(slots)))
        for sl in slots[R:]:   # fewer replicas than before: their device buffers go
            sl.close()
        del slots[R:]
        return slots

    def lockstep_applies(self, fmaps):
        """Whether R replicas go through the batched solvers: a host-side decision on the bound maps, before anything is
        allocated.  No: a solver other than ``utilities.solver.broyden``, ``bw_solver = "gmres"`` without ``bw_gmres_lockstep`` or with
        a non-default ``bw_gmres_augment`` / ``bw_gmres_stall``, an
        untiled plan, ``n_layers > 1``, a bf16 pair history, both families in one call, a mixed plan without
        ``lin_neumann = "stored"``.  (Solvers of one call share one size class by construction: all are sized for the whole shard.)"""
        if self.config_deq["solver"] is not _solver.broyden or self.history_dtype() != torch.float32:
            return False
        if self.config_deq.get("bw_solver") is not None and not self.config_deq.get("bw_gmres_lockstep"):
            return False   # the GMRES adjoint solve takes its lockstep form only with the key (decided before the maps are looked at)
        if self._bw_gmres_opts() is not None:
            return False   # kept corrections / another stall ratio: the lockstep GMRES takes no options
        if any(not f.plan.tiled or f.weights.n_layers != 1 or not f.can_linearize() for f in fmaps):
            return False
        if any(bool(f.plan.mixed) != bool(fmaps[0].plan.mixed) for f in fmaps):
            return False
        return not fmaps[0].plan.mixed or all(f.lin_neumann == "stored" for f in fmaps)

    def fp_lockstep_applies(self, fmaps):
        """Whether the forward solves of these maps go through the lockstep Anderson / Picard solve: ``fp_lockstep`` is set (the
        solver is then ``anderson`` or ``forward_iteration``: checked when the model was made), more than one mesh, tiled plans of
        one family, single-layer weights.  A host-side decision, before anything is allocated; ``engine.fpiter_batchable`` is asked
        again by the solve itself."""
        if not self.config_deq.get("fp_lockstep") or len(fmaps) < 2:
            return False
        if any(not f.plan.tiled or f.weights.n_layers != 1 for f in fmaps):
            return False
        return all(bool(f.plan.mixed) == bool(fmaps[0].plan.mixed) for f in fmaps)

    def fp_lockstep_solve(self, fmaps):
        """The solver dicts of the lockstep forward solve of ``fmaps`` (``utilities.solver.lockstep_batch``), from each map's h0."""
        return _solver.lockstep_batch(self.config_deq["solver"], fmaps, self.config_deq["fw_tol"], self.config_deq["fw_thres"])

    def train_forward_replicas(self, H_inits, batches, generator=None):
        """``(list of new_H_star, list of jacobian_loss)`` for R replicas, each an independent fixed-point problem with its own
        Broyden matrix and stop test -- what the reference's ``DataParallel`` does with ``num_gpus = R``
        (dirichlet/psignn/main.py:106, training_class.py:156-159), on one GPU.  One autograd function over all replicas: the R
        forward solves run in lockstep (``engine.broyden_solve_batch``), the backward builds one linearisation per replica at its
        H* and solves the R adjoint equations in lockstep (``engine.broyden_solve_adjoint_batch``); in this mode the backward is
        therefore the linearised one whatever ``bw_linearize`` says (it is the only batched product), and the mixed family needs
        ``lin_neumann = "stored"``.  Where the lockstep does not apply (``lockstep_applies``: solver other than broyden, untiled
        plan, ``n_layers > 1``, bf16 history, both families, mixed without stored Neumann rows; or ``engine.shard_batchable`` /
        ``engine.adjoint_batchable`` say no) the replicas are solved one after the other through the single-mesh paths; the
        result has replica semantics either way.  With ``bw_solver = "gmres"`` the replicas are solved one after the other, forward
        and backward, each slot keeping its own GMRES handle and basis -- unless ``bw_gmres_lockstep`` is set: the lockstep route
        then applies under the same conditions, its backward solving the R adjoint systems by restarted GMRES in lockstep
        (``engine.gmres_solve_adjoint_batch``; the handles are sized for the shard) or, where ``engine.gmres_adjoint_batchable``
        says no, with the same handles one after the other.  The Jacobian regulariser stays per replica (``_JacLossFn``), its probes drawn
        in replica order from ``generator`` and kept as ``last_probes``; ``last_forward`` / ``last_backward`` are lists of the
        solver dicts, the CSV log lines are written per replica.

        Memory: every replica slot keeps its forward and its adjoint solver between steps, ``2 * thr * N_r * d`` floats each
        (``thr`` = ``fw_thres`` / ``bw_thres``, ``N_r`` the nodes of replica r's union batch), and one linearisation handle;
        they are keyed by plan, threshold and history dtype and closed when the key changes."""
        R = len(batches)
        if R == 0 or len(H_inits) != R:
            raise ValueError("train_forward_replicas: one H_init per batch, at least one batch")
        if torch.is_grad_enabled():
            nat.require_default_width(self.f.latent_dim, "training (the implicit backward)")
        if not torch.is_grad_enabled():   # validation: the existing branch, one replica after the other
            pairs, fw = [], []
            for h, b in zip(H_inits, batches):
                pairs.append(self.train_forward(h, b, generator=generator))
                fw.append(self.last_forward)
            self.last_forward = fw
            return [p[0] for p in pairs], [p[1] for p in pairs]
        named = list(self.f.named_parameters())
        names, params = tuple(n for n, _ in named), [p for _, p in named]
        fmaps = [self.f.bind(h.detach(), b) for h, b in zip(H_inits, batches)]
        slots = self._replica_slots(R)
        self.last_backward = [None] * R
        if self.lockstep_applies(fmaps):
            new_Hs = list(_DEQReplicasFn.apply(self, tuple(batches), names, *H_inits, *params))
        else:
            new_Hs, fw = [], []
            # fp_lockstep: the R forward solves (anderson / forward_iteration) in one lockstep solve; each slot's _DEQFn then takes
            # its solver dict instead of solving again, and the backward is the slot's own, as without the key
            pre = self.fp_lockstep_solve(fmaps) if self.fp_lockstep_applies(fmaps) else [None] * R
            for sl, h, b, o in zip(slots, H_inits, batches, pre):
                sl.sink = self.last_backward
                sl.presolved = o
                new_Hs.append(_DEQFn.apply(h, sl, b, names, *params))
                fw.append(sl.last_forward)
            self.last_forward = fw
        H_stars = [o["result"] for o in self.last_forward]
        self.last_probes, jac = [], []
        for f, h in zip(fmaps, H_stars):
            v = torch.randn(h.shape, device=h.device, generator=generator)
            self.last_probes.append(v)
            jac.append(_JacLossFn.apply(f, h, v, names, *params))
        return new_Hs, jac

    # ---- adjoint side of the reference's training variant (dirichlet/psignn/model.py:204-241), on the VJP kernel
    def _linearization(self, fmap, H_star):
        """Linearisation of ``fmap`` at H* (plan order), or None where the plan has no stored form (``can_linearize``).  Its
        device buffers are kept between calls on the same plan, like the adjoint solver's."""
        if not fmap.can_linearize():
            return None
        lin = getattr(self, "_bw_lin", None)
        want = fmap.plan.mixed and fmap.lin_neumann == "stored"
        if lin is None or lin.fmap.plan is not fmap.plan or lin.neumann_stored != want:
            if lin is not None:
                lin.close()
            lin = self._bw_lin = engine.Linearization(fmap, neumann=fmap.lin_neumann)
        lin.fmap = fmap   # this call's weights and boundary data
        return fmap.linearize_p(fmap.to_plan(H_star), lin)

    def _linearize_default(self, linearize):
        """None -> the ``bw_linearize`` config value; a bool as given; an ``engine.Linearization`` (already built at H*) as is."""
        if isinstance(linearize, engine.Linearization):
            return linearize
        return bool(self.config_deq.get("bw_linearize", False)) if linearize is None else bool(linearize)

    def _bw_gmres_opts(self):
        """``(augment, stall)`` of the GMRES adjoint solve when ``bw_gmres_augment`` / ``bw_gmres_stall`` hold a non-default value,
        else None (the solve without options)."""
        a, st = int(self.config_deq.get("bw_gmres_augment", 0)), float(self.config_deq.get("bw_gmres_stall", 0.5))
        return None if a == 0 and st == 0.5 else (a, st)

    def implicit_backward(self, H_star, H_init, batch, grad):
        """Solve y = J_f(H*)^T y + grad with the configured solver (the reference's backward hook, model.py:210-223):
        returns the solver dict; ``out["result"]`` is the gradient w.r.t. the fixed point's input.  With ``bw_linearize``
        the map is the transposed product of one linearisation of f at H* (where ``fmap.can_linearize()``).  With
        ``bw_solver = "gmres"`` the system is solved by restarted GMRES instead (``engine.DeviceGmres.solve_adjoint``, restart
        length ``bw_gmres_m``): ``bw_tol`` is its tolerance, ``bw_thres`` its budget of transposed products.  With a non-default
        ``bw_gmres_augment`` / ``bw_gmres_stall`` the solve is ``engine.DeviceGmresAug.solve_adjoint`` and the dict carries ``n_aug``."""
        nat.require_default_width(self.f.latent_dim, "implicit_backward")
        fmap = self.f.bind(H_init, batch)
        g = grad.contiguous()
        lin = self._linearization(fmap, H_star) if self._linearize_default(None) else None
        if self.config_deq.get("bw_solver") == "gmres":   # opt-in: the linear system by restarted GMRES, whatever config["solver"] is
            # handle and basis ((m + 1) * N * d floats) are kept between calls on the same plan, like the Broyden adjoint solver's state
            m = int(self.config_deq.get("bw_gmres_m", 50))
            opts = self._bw_gmres_opts()
            if opts is not None:   # kept corrections and / or another stall ratio: a handle with a ring, keyed by its size too
                key = (fmap.plan, m, opts[0], "aug")
                old = getattr(self, "_bw_gmres_key", None)
                if old is None or len(old) != 4 or old[0] is not key[0] or old[1:] != key[1:]:
                    if getattr(self, "_bw_gmres", None) is not None:
                        self._bw_gmres.close()
                    self._bw_gmres = engine.DeviceGmresAug(fmap.plan.N * engine.D, fmap.plan.device, m, augment=opts[0])
                    self._bw_gmres_key = key
                out = self._bw_gmres.solve_adjoint(fmap, H_star, g, self.config_deq["bw_tol"], self.config_deq["bw_thres"], lin=lin,
                                                   augment=opts[0], stall=opts[1])
                out.update(eps=self.config_deq["bw_tol"], threshold=self.config_deq["bw_thres"])
                return out
            key = (fmap.plan, m)
            old = getattr(self, "_bw_gmres_key", None)
            if old is None or len(old) != 2 or old[0] is not key[0] or old[1] != m:
                if getattr(self, "_bw_gmres", None) is not None:
                    self._bw_gmres.close()
                self._bw_gmres = engine.DeviceGmres(fmap.plan.N * engine.D, fmap.plan.device, m)
                self._bw_gmres_key = key
            out = self._bw_gmres.solve_adjoint(fmap, H_star, g, self.config_deq["bw_tol"], self.config_deq["bw_thres"], lin=lin)
            out.update(eps=self.config_deq["bw_tol"], threshold=self.config_deq["bw_thres"])
            return out
        if self.config_deq["solver"] is _solver.broyden:  # whole adjoint solve on the device
            # the solver state (2 * bw_thres * N * d floats) is kept between calls on the same plan: a training loop
            # would otherwise allocate and free it once per step
            key = (fmap.plan, self.config_deq["bw_thres"], self.history_dtype())
            old = getattr(self, "_bw_key", None)
            if old is None or old[0] is not key[0] or old[1:] != key[1:]:
                if getattr(self, "_bw_solver", None) is not None:
                    self._bw_solver.close()
                self._bw_solver = engine.DeviceBroyden(plan=fmap.plan, threshold=self.config_deq["bw_thres"], keep_trace=False,
                                                       history_dtype=key[2])
                self._bw_key = key
            sv = self._bw_solver
            out = sv.solve_adjoint(fmap, H_star, g, self.config_deq["bw_tol"], lin=lin)
            out.update(eps=self.config_deq["bw_tol"], threshold=self.config_deq["bw_thres"])
            return out
        if lin is not None:
            return self.config_deq["solver"](lambda y: fmap.from_plan(lin.vjp_p(fmap.to_plan(y))) + g, torch.zeros_like(g),
                                             threshold=self.config_deq["bw_thres"], eps=self.config_deq["bw_tol"])
        return self.config_deq["solver"](lambda y: fmap.vjp(H_star, y) + g, torch.zeros_like(g),
                                         threshold=self.config_deq["bw_thres"], eps=self.config_deq["bw_tol"])

    def _vjp_in_plan_order(self, fmap, H_star, linearize=False):
        """(vjp, to_plan, from_plan) working in plan order where the tiled VJP applies (saves the four permutation
        passes of the caller-order entry point per product; norms and inner products do not depend on the numbering).
        ``linearize``: the transposed product of one linearisation at H* where the plan has one (True), or of the given
        Linearization, built at H* by the caller."""
        if isinstance(linearize, engine.Linearization):
            lin = linearize
        else:
            lin = self._linearization(fmap, H_star) if linearize else None
        if lin is not None:
            return lin.vjp_p, fmap.to_plan, fmap.from_plan
        if fmap.plan.tiled:
            Hp = fmap.to_plan(H_star)
            return (lambda w: fmap.vjp_p(Hp, w)), fmap.to_plan, fmap.from_plan
        ident = lambda t: t
        return (lambda w: fmap.vjp(H_star, w)), ident, ident

    def jac_loss_estimate(self, H_star, H_init, batch, vecs=1, generator=None, probes=None, linearize=None):
        """Hutchinson estimate of tr(J^T J) / (N d) (model.py:416-435) with the VJP kernel.  ``probes``: the Gaussian
        vectors to use instead of drawing ``vecs`` of them (so that a test can fix them).  ``linearize``: None -> the
        ``bw_linearize`` config value; True / False; or a Linearization built at H*."""
        nat.require_default_width(self.f.latent_dim, "jac_loss_estimate")
        fmap = self.f.bind(H_init, batch)
        vjp, to_p, _ = self._vjp_in_plan_order(fmap, H_star, self._linearize_default(linearize))
        acc = 0.0
        n = vecs if probes is None else len(probes)
        for i in range(n):
            v = torch.randn(H_star.shape, device=H_star.device, generator=generator) if probes is None else probes[i]
            acc = acc + vjp(to_p(v)).norm() ** 2
        return acc / n / H_star.numel()

    def power_method(self, H_star, H_init, batch, n_iters=150, generator=None, v0=None, linearize=None):
        """Spectral-radius estimate of J by power iteration on v^T J (model.py:437-452).  ``v0``: start vector instead
        of a Gaussian draw.  ``linearize``: None -> the ``bw_linearize`` config value; True / False; or a Linearization
        built at H*."""
        nat.require_default_width(self.f.latent_dim, "power_method")
        fmap = self.f.bind(H_init, batch)
        vjp, to_p, from_p = self._vjp_in_plan_order(fmap, H_star, self._linearize_default(linearize))
        ev = to_p(torch.randn(H_star.shape, device=H_star.device, generator=generator) if v0 is None else v0)
        val = torch.zeros((), device=H_star.device)
        for _ in range(n_iters):
            vj = vjp(ev)
            val = (vj * ev).sum() / (ev * ev).sum()
            ev = vj / vj.norm()
        return from_p(ev), val.abs()


for _name in ("history_dtype", "_linearization", "_linearize_default", "_bw_gmres_opts", "implicit_backward"):   # (implicit_backward: both bw_solver routes)
    setattr(_ReplicaSlot, _name, getattr(DeepEquilibrium, _name))
del _name


# ----------------------------------------------------------------------------------------------
# models
# ----------------------------------------------------------------------------------------------
class _Base(nn.Module):
    MIXED = False

    def __init__(self, config):
        super().__init__()
        self.config = dict(config)
        bc = self.config.get("bc")
        self.mixed = self.MIXED if bc is None else (bc == "mixed")
        self.config.setdefault("solver", _solver.broyden)
        for k, v in (("fw_tol", 1e-5), ("fw_thres", 300), ("bw_tol", 1e-8), ("bw_thres", 300), ("path_logs", None)):
            self.config.setdefault(k, v)
        d = nat.check_width(self.config["latent_dim"])   # engine.SUPPORTED_WIDTHS; NativeError naming them otherwise
        self.autoencoder = Autoencoder(hidden_channels=[1, d, d], activation=nn.ReLU())
        self.config_deq = {k: self.config[k] for k in ("solver", "fw_tol", "fw_thres", "bw_tol", "bw_thres", "path_logs")}
        if "bw_linearize" in self.config:   # optional, like "bc": the transposed stored linearisation in the backward routes
            self.config_deq["bw_linearize"] = bool(self.config["bw_linearize"])
        if "lin_neumann" in self.config:   # optional: the stored linearisation keeps the mixed family's Neumann rows too
            self.config_deq["lin_neumann"] = engine.check_lin_neumann(self.config["lin_neumann"])   # (ValueError otherwise)
        if "jac_backward" in self.config:   # optional: the Jacobian regulariser's backward on the tile kernels where the plan has them
            self.config_deq["jac_backward"] = engine.check_jac_backward(self.config["jac_backward"])   # (ValueError otherwise)
        if "bw_solver" in self.config or "bw_gmres_m" in self.config:   # optional: restarted GMRES for the implicit backward
            m = self.config.get("bw_gmres_m", min(50, int(self.config["bw_thres"])))   # (50: the restart length at which the CPU probe's error matched Broyden's)
            self.config_deq["bw_solver"] = engine.check_bw_solver(self.config.get("bw_solver"), m, self.config["bw_thres"])   # (NativeError otherwise)
            self.config_deq["bw_gmres_m"] = m
        if "bw_gmres_lockstep" in self.config:   # optional: replicas with bw_solver = "gmres" solve their adjoint systems in lockstep
            self.config_deq["bw_gmres_lockstep"] = engine.check_bw_gmres_lockstep(self.config["bw_gmres_lockstep"],
                                                                                 self.config.get("bw_solver"))   # (NativeError otherwise)
        if "bw_gmres_augment" in self.config or "bw_gmres_stall" in self.config:   # optional: LGMRES restarts / the stall ratio of the GMRES adjoint solve
            a, st = engine.check_bw_gmres_aug(self.config.get("bw_gmres_augment"), self.config.get("bw_gmres_stall"),
                                              self.config.get("bw_solver"), self.config_deq.get("bw_gmres_m"))   # (NativeError otherwise)
            if "bw_gmres_augment" in self.config:
                self.config_deq["bw_gmres_augment"] = a
            if "bw_gmres_stall" in self.config:
                self.config_deq["bw_gmres_stall"] = st
        if "fp_lockstep" in self.config:   # optional: shards solved by anderson / forward_iteration run in lockstep
            self.config_deq["fp_lockstep"] = engine.check_fp_lockstep(self.config["fp_lockstep"], self.config["solver"],
                                                                     (_solver.anderson, _solver.forward_iteration))   # (NativeError otherwise)
        if "broyden_history_dtype" in self.config:   # optional: bf16 storage of the Broyden pairs (utilities.solver.broyden only)
            engine.history_code(self.config["broyden_history_dtype"])   # (ValueError for any other dtype)
            self.config_deq["broyden_history_dtype"] = self.config["broyden_history_dtype"]
        self.deqdss = DeepEquilibrium(
            function=Function(n_layers=self.config["n_layers"], latent_dim=d, edge_features_dim=3,
                              second_member_dim=3 if self.mixed else 2, activation=nn.ReLU(), mixed=self.mixed),
            config_deq=self.config_deq)
        self.deqdss.f.lin_neumann = self.config_deq.get("lin_neumann", "direct")
        self.deqdss.f.jac_backward = self.config_deq.get("jac_backward", "gather")
        self.mse_loss = nn.MSELoss()

    # -- helpers -------------------------------------------------------------------------------
    def _dirichlet_index(self, batch):
        t = batch.tags[:, 1] if self.mixed else batch.tags.reshape(batch.tags.shape[0], -1)[:, 0]
        return torch.where(t == 1)[0]

    def residual_loss(self, u, batch):
        """mean((A u - y)^2), A incl. the diagonal (model.py:157-167)."""
        r = engine.residual_autograd(engine.plan_for(batch), u, batch.y, batch.a_ij)
        return torch.mean(r ** 2)

    @torch.no_grad()
    def _solve(self, batch):
        nat.require_cuda(batch.x, "batch.x")
        h_initial = self.autoencoder.encoder(batch.x)
        out = self.deqdss(h_initial, batch)
        return h_initial, out

    @torch.no_grad()
    def _diagnostics(self, u_final, h_final, batch, key_dir, idx=None):
        enc = self.autoencoder.encoder(u_final)
        if idx is None:
            idx = self._dirichlet_index(batch)
        return {
            "residual_loss": self.residual_loss(u_final, batch),
            "encoder_loss": self.mse_loss(enc, h_final),
            "autoencoder_loss": self.mse_loss(self.autoencoder.decoder(enc), u_final),
            "mse_loss": self.mse_loss(u_final, batch.sol),
            key_dir: self.mse_loss(u_final[idx, :], batch.x[idx, :]),
        }

    @torch.no_grad()
    def inference(self, batch):
        """u_final only (dirichlet/psignn/model.py:99-107)."""
        _, out = self._solve(batch)
        return self.autoencoder.decoder(out["result"])

    @torch.no_grad()
    def _iterative(self, batch):
        """tests/model_psignn.py:145-194 ≡ dirichlet/psignn/model.py:109-155."""
        out_dic = {"sol_dic": [], "res_dic": [], "mse_dic": [], "bound_mse_dic": [], "inter_mse_dic": [], "nstep": []}
        if self.mixed:
            ib = torch.where(batch.tags[:, 1] == 1)[0]
            ii = torch.where(batch.tags[:, 0] == 1)[0]
        else:
            ib = torch.where(batch.tags == 1)[0]
            ii = torch.where(batch.tags == 0)[0]

        def record(u):
            out_dic["sol_dic"].append(u.cpu())
            out_dic["res_dic"].append(self.residual_loss(u, batch).cpu().item())
            out_dic["mse_dic"].append(torch.mean((u - batch.sol) ** 2).cpu().item())
            out_dic["bound_mse_dic"].append(torch.mean((u[ib, :] - batch.sol[ib, :]) ** 2).cpu().item())
            out_dic["inter_mse_dic"].append(torch.mean((u[ii, :] - batch.sol[ii, :]) ** 2).cpu().item())

        record(batch.x)
        _, out_fw = self._solve(batch)
        for h_star in out_fw["xest_trace"]:
            record(self.autoencoder.decoder(h_star))
        out_dic["nstep"] = out_fw["nstep"]
        return out_dic


class ModelPSIGNN(_Base):
    """tests/model_psignn.py:28-112: ``forward(batch) -> (u_final, loss_dic incl. 'nsteps')``."""

    @torch.no_grad()
    def forward(self, batch):
        _, out = self._solve(batch)
        h_final = out["result"]
        u_final = self.autoencoder.decoder(h_final)
        loss_dic = self._diagnostics(u_final, h_final, batch, "mse_dirichlet_loss")
        loss_dic["nsteps"] = out["nstep"]
        return u_final, loss_dic


class ModelPSIGNNIterative(_Base):
    """tests/model_psignn.py:114-206: per-iterate diagnostics dictionary."""

    def forward(self, batch):
        return self._iterative(batch)


class ModelDEQDSS(_Base):
    """dirichlet/psignn/model.py:28-167: ``forward`` (training: differentiable, implicit backward; eval: diagnostics),
    ``inference``, ``iterative_inference``."""

    def forward(self, batch):
        # At a width other than engine.D there is forward inference only: no training step, and not this method's validation
        # branch either (its jacobian_loss is a transposed Jacobian product) -- ``inference`` / ``iterative_inference`` are the
        # entry points there.  Decided here, before anything is launched.
        nat.require_default_width(self.config["latent_dim"], "ModelDEQDSS.forward (training step / validation with jacobian_loss; "
                                  "use inference() or iterative_inference())")
        if isinstance(batch, (list, tuple)):
            return self._forward_replicas(list(batch))
        if self.training and torch.is_grad_enabled():
            return self._train_forward(batch)
        with torch.no_grad():  # validation branch of DeepEquilibrium.forward (model.py:227-241): one more f on H*
            nat.require_cuda(batch.x, "batch.x")
            h_initial = self.autoencoder.encoder(batch.x)
            h_final, jacobian_loss = self.deqdss.train_forward(h_initial, batch)
            u_final = self.autoencoder.decoder(h_final)
            # ModelDEQDSS.forward is ONE function for both modes: its Dirichlet statistic uses where(tags == 1)[0] also on
            # the mixed family's one-hot (N, 3) tags, i.e. every row (mixed/psignn/model.py:87) -- as _train_forward below
            loss_dic = self._diagnostics(u_final, h_final, batch, "mse_dirichlet", idx=torch.where(batch.tags == 1)[0])
            loss_dic["jacobian_loss"] = jacobian_loss
            return u_final, loss_dic

    def _train_forward(self, batch):
        """dirichlet/psignn/model.py:58-99.  Every term carries the gradient it has in the reference: residual_loss
        through decoder, implicit DEQ backward, f parameters and encoder; encoder_loss into the encoder;
        autoencoder_loss into the decoder only (the encoder output is detached there)."""
        nat.require_cuda(batch.x, "batch.x")
        ae = self.autoencoder
        h_initial = ae.encoder(batch.x)
        h_final, jacobian_loss = self.deqdss.train_forward(h_initial, batch)
        u_final = ae.decoder(h_final)
        residual_loss = self.residual_loss(u_final, batch)
        u_d, h_d = u_final.detach(), h_final.detach()
        encoder_loss = self.mse_loss(ae.encoder(u_d), h_d)
        autoencoder_loss = self.mse_loss(ae.decoder(ae.encoder(u_d).detach()), u_d)
        # model.py:87 in BOTH families: where(tags == 1)[0]; on the mixed family's one-hot (N, 3) tags that is every row
        idx = torch.where(batch.tags == 1)[0]
        loss_dic = {"residual_loss": residual_loss, "jacobian_loss": jacobian_loss, "encoder_loss": encoder_loss,
                    "autoencoder_loss": autoencoder_loss, "mse_loss": self.mse_loss(u_final, batch.sol),
                    "mse_dirichlet": self.mse_loss(u_final[idx, :], batch.x[idx, :])}
        return u_final, loss_dic

    def _forward_replicas(self, batches):
        """A list of R union batches = the R replicas of the reference's ``DataParallel`` call (dirichlet/psignn/main.py:106):
        ``(list of u_final, loss_dic)`` with every value of ``loss_dic`` stacked to shape ``(R,)`` -- what PyG's gather hands
        the trainer, whose ``.mean()`` makes the parameter gradient the mean of the replicas' gradients.  Training mode with
        gradients: ``DeepEquilibrium.train_forward_replicas``; otherwise each batch through the validation branch."""
        if len(batches) == 0:
            raise ValueError("forward received an empty list of batches")
        if not (self.training and torch.is_grad_enabled()):
            outs = [self.forward(b) for b in batches]
            keys = outs[0][1].keys()
            return [u for u, _ in outs], {k: torch.stack([torch.as_tensor(d[k], device=u.device) for u, d in outs]) for k in keys}
        ae = self.autoencoder
        for b in batches:
            nat.require_cuda(b.x, "batch.x")
        h_inits = [ae.encoder(b.x) for b in batches]
        h_finals, jac = self.deqdss.train_forward_replicas(h_inits, batches)
        us, dics = [], []
        for batch, h_final, jacobian_loss in zip(batches, h_finals, jac):   # per replica the terms of _train_forward
            u_final = ae.decoder(h_final)
            u_d, h_d = u_final.detach(), h_final.detach()
            idx = torch.where(batch.tags == 1)[0]
            dics.append({"residual_loss": self.residual_loss(u_final, batch), "jacobian_loss": jacobian_loss,
                         "encoder_loss": self.mse_loss(ae.encoder(u_d), h_d),
                         "autoencoder_loss": self.mse_loss(ae.decoder(ae.encoder(u_d).detach()), u_d),
                         "mse_loss": self.mse_loss(u_final, batch.sol),
                         "mse_dirichlet": self.mse_loss(u_final[idx, :], batch.x[idx, :])})
            us.append(u_final)
        return us, {k: torch.stack([d[k] for d in dics]) for k in dics[0]}

    def iterative_inference(self, batch):
        return self._iterative(batch)
