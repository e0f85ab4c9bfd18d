/*
 * psignn_hip.h — C ABI of libpsignn_hip.so, the MI355X (gfx950) implementation of the PSI-GNN
 * fixed-point inference hot path.
 *
 * The reference (mnastorg/PSI-GNN) has no FFI layer: its hot path is Python calling
 * torch_geometric / torch_sparse / ATen kernels.  Each entry point below replaces one such
 * call site; the citation after "replaces:" is the reference file:line (relative to the
 * reference repository root).  All pointers named d_* are DEVICE pointers (hipMalloc'ed or
 * owned by any framework's allocator); h_* are host pointers.  `stream` is a hipStream_t
 * passed as void* (NULL = default stream).  Every function returns 0 on success or a negative
 * PSIGNN_E* code; psignn_last_error() returns a message for the calling thread.
 *
 * Unless stated otherwise calls are asynchronous on `stream` and perform no host sync.
 * Tensors are dense row-major float32; node states are (N, d) — the latent width d is fixed at
 * compile time (PSIGNN_D).  d = 10 is the only value the reference ever trains (SURVEY.md "d") and
 * is what libpsignn_hip.so is built for; libpsignn_hip_d<w>.so is the same source built with
 * -DPSIGNN_D=<w> (even widths from 4 to 16) and holds the forward-inference entry points only.
 */
#ifndef PSIGNN_HIP_H
#define PSIGNN_HIP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef PSIGNN_D
#define PSIGNN_D 10            /* latent_dim */
#endif
#define PSIGNN_EDGE_F 3        /* edge_features_dim */

#define PSIGNN_OK 0
#define PSIGNN_EINVAL (-1)     /* bad argument / shape */
#define PSIGNN_EHIP (-2)       /* HIP runtime error */
#define PSIGNN_EINDEX (-3)     /* edge index out of range */
#define PSIGNN_ENOMEM (-4)

const char* psignn_last_error(void);
int psignn_version(void);
/* The latent width this library was compiled for (PSIGNN_D): 10 for libpsignn_hip.so.  A weight buffer, a state or a
 * solver made for one width must never reach a library of another; psignn_weights_size() reports this width's total. */
int psignn_latent_dim(void);
/* Re-read the PSIGNN_* environment knobs at their next use (they are cached after the first read).  The knobs select
 * alternative forms of a kernel for A/B measurements and tests (MFMA stage 1, Hilbert tiling, gather kernels for the mixed
 * family, ...); a normal run sets none of them.  No reference counterpart. */
void psignn_reload_knobs(void);

/* ------------------------------------------------------------------------------------------
 * Mesh plan: everything iteration-invariant, computed once per mesh on the device.
 *
 * replaces: torch_geometric.utils.remove_self_loops executed twice per f call
 *           (dirichlet/psignn/model.py:342,360), torch.where(tags == 1) re-run every f call
 *           (model.py:281; mixed/psignn/model.py:218-219), and the COO->CSR conversion inside
 *           SparseTensor(...) (model.py:159-163).
 *
 * Layout built (all int32 / float32, device memory owned by the plan):
 *   csr: non-self edges grouped by row  r = edge_index[0]  (aggregation side of Phi_from)
 *   csc: non-self edges grouped by col  c = edge_index[1]  (aggregation side of Phi_to)
 *   inside a group edges are ordered by (other endpoint, original edge id) — a canonical order
 *   independent of the input edge order; edge_attr is stored once per ordering;
 *   full CSR of A (self loops included, a_ij values) for the residual SpMV;
 *   node flags: bit0 = Dirichlet, bit1 = Neumann.
 * ------------------------------------------------------------------------------------------ */
typedef struct psignn_plan psignn_plan_t;

/* tags: (N, tags_cols) float32 with tags_cols = 1 (dirichlet: tags[:,0]==1 -> Dirichlet) or
 * 3 (mixed one-hot [interior, dirichlet, neumann]).  d_a_ij may be NULL (no residual SpMV).
 * d_pos: (N,2) node coordinates (batch.pos) or NULL; used only to renumber nodes into spatially
 * compact tiles (speed, never results).  tile_target: nodes per tile (0 = default, < 0 = no tiles).
 * Synchronous: returns after the plan is complete (a few small device->host reads). */
int psignn_plan_create(psignn_plan_t** out, int64_t n_nodes, int64_t n_edges,
                       const int64_t* d_edge_index /* (2, E) */, const float* d_edge_attr /* (E,3) */,
                       const float* d_a_ij /* (E) or NULL */, const float* d_tags, int tags_cols,
                       const float* d_pos, int tile_target, void* stream);
void psignn_plan_destroy(psignn_plan_t* plan);

/* Tile structures: when present, solver state is kept in "plan order"
 * (nodes renumbered tile by tile).  psignn_plan_permute moves (N, cols) float rows between the
 * caller's numbering and plan order: to_plan = 1: dst[new] = src[perm[new]]; 0: dst[old] = src[inv[old]].
 * On an untiled plan it is a copy. */
int psignn_plan_is_tiled(const psignn_plan_t* plan);
int64_t psignn_plan_num_tiles(const psignn_plan_t* plan);
int64_t psignn_plan_ell_rows(const psignn_plan_t* plan);      /* 64-lane ELL slot-rows (padding included) */
int psignn_plan_max_tile_rows(const psignn_plan_t* plan);     /* max tile + halo rows staged in LDS */
int psignn_plan_permute(const psignn_plan_t* plan, const float* d_src, int cols, float* d_dst, int to_plan,
                        void* stream);

int64_t psignn_plan_num_nodes(const psignn_plan_t* plan);
int64_t psignn_plan_num_edges(const psignn_plan_t* plan);          /* E, as given */
int64_t psignn_plan_num_nonself_edges(const psignn_plan_t* plan);  /* E' */

/* Copy one plan array to host memory (tests: bit-exact comparison with the numpy oracle).
 * which: 0 csr_ptr(N+1 i32) 1 csr_nbr(E' i32) 2 csr_eid(E' i32) 3 csc_ptr 4 csc_nbr 5 csc_eid
 *        6 node_flags (N u8) 7 csr_attr (E'*3 f32) 8 csc_attr 9 a_ptr (N+1 i32) 10 a_col (E i32)
 *        11 a_val (E f32); tiled plans only: 12 perm (N i32, perm[new] = old) 13 tile_ptr (T+1 i32)
 *        14 halo_cnt (T i32) 15 halo (T*512 i32) 16 slice_off (S+1 i32) 17 slice_deg (S u8)
 *        18 ell (rows*64*4 u32: pair-merged neighbour slots) 20 tile_slice (T+1 i32).  Synchronous. */
int psignn_plan_export(const psignn_plan_t* plan, int which, void* h_dst, size_t dst_bytes);

/* ------------------------------------------------------------------------------------------
 * Weights: one flat float32 device buffer in the order documented in DESIGN.md §weights
 * (nn.Linear (out,in) row-major blocks, concatenated).  psignn_weights_size() gives its length.
 * replaces: the nn.Module parameter tensors of Function / Phi_to / Phi_from / MLP
 *           (dirichlet/psignn/model.py:265-277,316-368; mixed/psignn/model.py:198-214).
 * ------------------------------------------------------------------------------------------ */
int64_t psignn_weights_size(int mixed, int n_layers);

/* ------------------------------------------------------------------------------------------
 * f_theta: one application of the GNN block.
 * replaces: Function.forward (dirichlet/psignn/model.py:279-300 == tests/model_psignn.py:269-290;
 *           mixed/psignn/model.py:216-245) including both/all three MessagePassing.propagate
 *           passes, the gated update MLP, LayerNorm and the Dirichlet/Neumann row handling.
 * d_prb: (N,2) dirichlet / (N,3) mixed.  d_normals: (N,2) mixed only, else NULL.
 * d_work: scratch of psignn_f_workspace_floats(plan) floats (what each form keeps in it: the f-workspace views of
 * csrc/workspace.h -- ws::FFwd, ws::FVjp, ws::Adapter; every workspace of this header is laid out there, by the function that
 * also answers its size query).  d_out must not alias d_h.
 * ------------------------------------------------------------------------------------------ */
int64_t psignn_f_workspace_floats(const psignn_plan_t* plan);

/* Extra scratch the derivatives of a multi-layer block need: dirichlet, the layer states h_1..h_{L-1}, the tangents and
 * cotangents carried between layers and a single-layer weight view, (4 n_layers + 1) * N * 10 + 4096 floats (ws::LayerWork); mixed (whose
 * iterated layer is the last one), the weight view alone; 0 for single-layer blocks.  A derivative entry point that takes
 * d_work is then given its own workspace (psignn_f_workspace_floats for psignn_f_jvp / _jvp_pw / _vjp / _vjp_p,
 * psignn_f_param_vjp_workspace_floats for the parameter VJPs, psignn_f_vjp_backward_workspace_floats for the backward of the
 * VJP) + psignn_f_layers_workspace_floats(plan, n_layers) floats.
 * Multi-layer dirichlet blocks: those entry points do not take h_initial; the Dirichlet rows of the intermediate layer
 * states are taken from d_h's own Dirichlet rows, which is exact wherever they equal h_initial's (every state f returns,
 * h_initial itself, a fixed point). */
int64_t psignn_f_layers_workspace_floats(const psignn_plan_t* plan, int n_layers);
int psignn_f_forward(const psignn_plan_t* plan, const float* d_weights, int n_layers,
                     const float* d_h, const float* d_h_initial, const float* d_prb,
                     const float* d_normals, float* d_out, float* d_work, void* stream);

/* Same, with h, h_initial, prb, normals and out already in plan order (no permutation passes):
 * the form iterative callers use after one psignn_plan_permute per tensor. */
int psignn_f_forward_p(const psignn_plan_t* plan, const float* d_weights, int n_layers,
                       const float* d_h, const float* d_h_initial, const float* d_prb,
                       const float* d_normals, float* d_out, float* d_work, void* stream);

/* n successive applications x <- f(x) in plan order without host involvement between them.
 * replaces: the loop body of forward_iteration (utilities/solver.py:301-341) minus its per-step norms.
 * d_x: x_0 on entry, x_n on return; d_tmp: a second (N, d) buffer. */
int psignn_picard_p(const psignn_plan_t* plan, const float* d_weights, int n_layers, float* d_x, float* d_tmp,
                    const float* d_h_initial, const float* d_prb, const float* d_normals, float* d_work, int n,
                    void* stream);

/* Single message-passing aggregation (tests / diagnostics): which = 0 Phi_to, 1 Phi_from,
 * 2 Phi_neumann (mixed).  replaces: Phi_to.forward / Phi_from.forward (model.py:334-368). */
int psignn_phi(const psignn_plan_t* plan, const float* d_weights, int n_layers, int layer, int which,
               const float* d_h, float* d_out, float* d_work, void* stream);

/* Jacobian-vector product of f at h along v (analytic, no finite differences).
 * replaces: nothing executable in the reference (scipy.optimize.newton_krylov is imported at
 *           utilities/solver.py:6 but never called); it is the transpose of the VJP that
 *           autograd.grad(new_H, H, v) computes at model.py:214,432,449. */
int psignn_f_jvp(const psignn_plan_t* plan, const float* d_weights, int n_layers,
                 const float* d_h, const float* d_prb, const float* d_normals,
                 const float* d_v, float* d_out, float* d_work, void* stream);

/* Linearisation of f at a fixed state h, for Krylov solvers that apply J_f(h) to many vectors (Newton-Krylov, BASELINE config 5):
 * psignn_lin_build evaluates the value path of f once and stores what the Jacobian needs (relu masks of every edge direction as
 * wave-level bit masks, per-node gate / update / LayerNorm quantities); psignn_lin_jvp then applies J_f(h) as a linear operator,
 * at about half the cost of psignn_f_jvp.  Tiled plans; dirichlet: single-layer blocks; mixed (d_normals_plan required; the tiles
 * holding Neumann nodes run the direct kernel at a copy of the state kept by the build, unless the handle stores the Neumann rows:
 * psignn_lin_create_opts below).  h, prb, normals, v, out in PLAN order
 * (psignn_plan_permute).  The handle keeps a pointer to the plan: destroy it before the plan.
 * replaces: nothing executable in the reference (see psignn_f_jvp); same product as psignn_f_jvp up to fp32 summation order. */
typedef struct psignn_lin psignn_lin_t;
int psignn_lin_create(psignn_lin_t** out, const psignn_plan_t* plan);
void psignn_lin_destroy(psignn_lin_t* lin);
size_t psignn_lin_bytes(const psignn_lin_t* lin);
int psignn_lin_build(psignn_lin_t* lin, const float* d_weights, int n_layers, const float* d_h_plan, const float* d_prb_plan,
                     const float* d_normals_plan, void* stream);
int psignn_lin_jvp(const psignn_lin_t* lin, const float* d_weights, int n_layers, const float* d_v_plan, float* d_out_plan,
                   void* stream);
/* Transposed product out = J_f(h)^T w of the same stored linearisation (the exact transpose of psignn_lin_jvp's operator: same masks,
 * same per-node records), w and out in PLAN order.  Dirichlet plans: one kernel per product; the first call after a build also fills
 * a transposed copy of the slot masks, the first call of the handle also allocates it and a reverse slot map (psignn_lin_bytes then
 * counts them; the build and psignn_lin_jvp do not use them).  A handle is single-stream: its build and its products (which may write
 * the handle's transposed masks on the first call after a build) must be issued on one stream, or ordered by the caller.  A plan whose
 * slots the reverse map cannot pair is refused (PSIGNN_EINVAL) rather than answered without some edges.  Mixed plans: the tiled VJP
 * at the state kept by the build (no cheaper than psignn_f_vjp_p there; psignn_lin_create_opts below stores the Neumann rows instead), d_work =
 * psignn_f_workspace_floats(plan) floats of scratch; dirichlet plans ignore d_work.  Errors: not built, in-place, wrong depth.
 * replaces: torch.autograd.grad(new_H, H, v) at one fixed state H*: the backward hook (dirichlet/psignn/model.py:210-223), the power
 *           method (:437-452) and the Hutchinson estimate (:416-435); same product as psignn_f_vjp_p up to fp32 summation order. */
int psignn_lin_vjp(const psignn_lin_t* lin, const float* d_weights, int n_layers, const float* d_w_plan, float* d_out_plan,
                   float* d_work, void* stream);
/* psignn_lin_create with options.  neumann_stored = 0 is psignn_lin_create.  neumann_stored = 1 on a mixed plan stores the Neumann
 * rows as well: the build runs every tile through the build kernel (a Neumann row keeps the relu masks of Phi_neumann's first layer
 * on its OUT slots in the Phi_from bit field of its slot dwords, and 1 / sqrt(var + eps), the hidden relu mask of update_neumann and
 * y_hat in its node record), psignn_lin_jvp applies that stored operator on the tiles holding Neumann nodes too (no direct kernel),
 * and psignn_lin_vjp is its exact transpose from the same dwords and records (no tiled VJP; d_work is accepted and ignored).  Such a
 * handle keeps no copy of h / prb / normals (psignn_lin_bytes reports what is held).  On a dirichlet plan the option is accepted and
 * changes nothing.  psignn_lin_neumann_stored: 1 when the handle stores the Neumann rows (mixed plan and option on), else 0.
 * replaces: torch.autograd.grad(new_H, H, v) at one fixed state of the mixed family, whose Neumann rows are
 *           LayerNorm(update_neumann([h, Phi_neumann(h), prb, normal])) (mixed/psignn/model.py:225,233-236,241): the backward hook,
 *           the power method and the Hutchinson estimate of mixed/psignn/model.py; same products as psignn_f_jvp / psignn_f_vjp_p
 *           up to fp32 summation order. */
int psignn_lin_create_opts(psignn_lin_t** out, const psignn_plan_t* plan, int neumann_stored);
int psignn_lin_neumann_stored(const psignn_lin_t* lin);

/* Vector-Jacobian product out = w^T (df/dh) at h (both families), as two gather passes over the plan's
 * CSR/CSC lists (no atomics).  d_normals: (N,2) for mixed plans, else NULL.
 * replaces: torch.autograd.grad(new_H_star, H_star, y) inside the implicit backward hook
 *           (dirichlet/psignn/model.py:210-223), jac_loss_estimate (:416-435) and power_method (:437-452). */
int psignn_f_vjp(const psignn_plan_t* plan, const float* d_weights, int n_layers, const float* d_h,
                 const float* d_prb, const float* d_normals, const float* d_w, float* d_out, float* d_work,
                 void* stream);

/* JVP with h, prb, normals, v and out in plan order (the tiled LDS-staged kernel: single-layer dirichlet plans, and
 * mixed plans of any depth, whose iterated layer is the last one).  d_normals: (N,2) in plan order for mixed plans, else NULL. */
int psignn_f_jvp_p(const psignn_plan_t* plan, const float* d_weights, int n_layers, const float* d_h, const float* d_prb,
                   const float* d_normals, const float* d_v, float* d_out, void* stream);

/* Same with a workspace: any depth.  A multi-layer dirichlet block evaluates its layer states into d_work
 * (psignn_f_workspace_floats + psignn_f_layers_workspace_floats floats) and chains the single-layer JVPs; other blocks
 * on tiled plans run psignn_f_jvp_p and may pass d_work = NULL.  Plans without tiles: plan order is the caller's order, and
 * d_work is psignn_f_jvp's (never NULL). */
int psignn_f_jvp_pw(const psignn_plan_t* plan, const float* d_weights, int n_layers, const float* d_h, const float* d_prb,
                    const float* d_normals, const float* d_v, float* d_out, float* d_work, void* stream);

/* Same with h, prb, w and out in plan order (tiled kernels where the plan has tiles; the form the adjoint solve uses). */
int psignn_f_vjp_p(const psignn_plan_t* plan, const float* d_weights, int n_layers, const float* d_h,
                   const float* d_prb, const float* d_normals, const float* d_w, float* d_out, float* d_work,
                   void* stream);

/* Parameter gradient  w^T (d f / d theta)  at h (plan order; tiled dirichlet plans, any depth), together with
 * w^T (d f / d h) -> d_out_h.  Replaces loss.backward() through new_H = f(H*, H_init, batch) with the hooked
 * cotangent (dirichlet/psignn/model.py:203-225, training_class.py:150-163).  d_grad receives
 * psignn_param_grad_size(mixed, n_layers) floats laid out like the leading (un-derived) section of the packed
 * weights: shared{ln_gamma, ln_beta, alpha_w, alpha_b} | phi_to{W1,b1,W2,b2} | phi_from | update{U1,c1,U2,c2};
 * derived (fold) slots stay zero.  d_work: psignn_f_param_vjp_workspace_floats(plan) floats (ws::pv_work, ws::pv_adapter). */
int64_t psignn_param_grad_size(int mixed, int n_layers);
int64_t psignn_f_param_vjp_workspace_floats(const psignn_plan_t* plan);
/* the same in the caller's numbering and for every plan and depth: tiled plans of both families run the tile kernels in
 * record mode (mixed family: d_normals required; d_grad then also covers phi_neumann{W1,b1,W2,b2} |
 * update_neumann{N1,nb1,N2,nb2}; mixed/psignn/model.py:216-245 under loss.backward()), untiled plans the global-gather kernels. */
int psignn_f_param_vjp(const psignn_plan_t* plan, const float* d_weights, int n_layers, const float* d_h,
                       const float* d_prb, const float* d_normals, const float* d_w, float* d_grad, float* d_out_h,
                       float* d_work, void* stream);
/* Same, and d_out_init (N, 10), may be NULL: the gradient w.r.t. h_initial -- the Dirichlet rows of the cotangent on the output
 * of every layer (a multi-layer dirichlet block copies those rows from h_initial after every layer, model.py:298; otherwise the
 * Dirichlet rows of d_w).  Any depth: n_layers > 1 needs psignn_f_param_vjp_workspace_floats + psignn_f_layers_workspace_floats
 * floats of d_work (also for psignn_f_param_vjp / _p and psignn_f_vjp_backward at that depth).  A multi-layer mixed block
 * receives gradients for its last layer only; the earlier layers' slots are zero (mixed/psignn/model.py:221-245). */
int psignn_f_param_vjp_ex(const psignn_plan_t* plan, const float* d_weights, int n_layers, const float* d_h, const float* d_prb,
                          const float* d_normals, const float* d_w, float* d_grad, float* d_out_h, float* d_out_init,
                          float* d_work, void* stream);
int psignn_f_param_vjp_p(const psignn_plan_t* plan, const float* d_weights, int n_layers, const float* d_h,
                         const float* d_prb, const float* d_w, float* d_grad, float* d_out_h, float* d_work,
                         void* stream);

/* Backward of the VJP: gradient of  phi = gbar . (J_f(h)^T v) = v^T J_f(h) gbar  (gbar held constant) w.r.t. the
 * parameters (d_grad, layout above) and w.r.t. h (d_grad_h, (N,10)).  Replaces autograd's double backward through
 * jac_loss_estimate -- autograd.grad(f0, z0, v, create_graph=True), dirichlet/psignn/model.py:416-435 -- when the
 * Jacobian regulariser is part of the loss (jac_weight, training_class.py:156-159): with g = J^T v and
 * jac_loss = |g|^2 / (N d), pass gbar = (d loss / d jac_loss) * 2 g / (N d).  Caller's numbering; blocks of both
 * families and any depth (multi-layer: d_work grows by psignn_f_layers_workspace_floats) (mixed: d_normals required, d_grad also covers phi_neumann | update_neumann).  d_work: psignn_f_vjp_backward_workspace_floats(plan) floats (ws::JrWork). */
int64_t psignn_f_vjp_backward_workspace_floats(const psignn_plan_t* plan);
int psignn_f_vjp_backward(const psignn_plan_t* plan, const float* d_weights, int n_layers, const float* d_h,
                          const float* d_prb, const float* d_normals, const float* d_v, const float* d_gbar, float* d_grad,
                          float* d_grad_h, float* d_work, void* stream);

/* The same gradient on the tile structures, every node tensor (d_h, d_prb, d_v, d_gbar, d_grad_h) in PLAN order
 * (psignn_plan_permute) -- the double backward loss.backward() runs through jac_loss_estimate,
 * dirichlet/psignn/model.py:416-435, training_class.py:156-159 -- as two tile kernels and the record reduction.
 * psignn_f_vjp_backward_tiled_ok: 1 where this form applies (tiled plan of the dirichlet family, n_layers == 1), else 0
 * (also for a NULL plan); where it is 0, psignn_f_vjp_backward_p is an argument error and launches nothing.  d_grad as above;
 * d_work: psignn_f_vjp_backward_p_workspace_floats(plan) floats (ws::JrWork, tile form). */
int psignn_f_vjp_backward_tiled_ok(const psignn_plan_t* plan, int n_layers);
int64_t psignn_f_vjp_backward_p_workspace_floats(const psignn_plan_t* plan);
int psignn_f_vjp_backward_p(const psignn_plan_t* plan, const float* d_weights, int n_layers, const float* d_h,
                            const float* d_prb, const float* d_v, const float* d_gbar, float* d_grad, float* d_grad_h,
                            float* d_work, void* stream);

/* Backward of psignn_mlp2 and of psignn_residual: what autograd runs for the autoencoder and residual terms of
 * the training loss (dirichlet/psignn/model.py:58-99).  d_gflat = gradients of [W1 | b1 | W2 | b2];
 * d_gx (n, din) may be NULL.  psignn_residual_t: out = A^T r with the caller's a_ij (E floats, edge_index order). */
int64_t psignn_mlp2_backward_workspace_floats(int64_t n);
int psignn_mlp2_backward(const float* d_x, const float* d_gy, int64_t n, int din, int hid, int dout, const float* d_w1,
                         const float* d_b1, const float* d_w2, float* d_gx, float* d_gflat, float* d_work, void* stream);
int psignn_residual_t(const psignn_plan_t* plan, const float* d_a_ij, const float* d_r, float* d_out, void* stream);

/* DS-GPS, the unrolled recurrent baseline (dirichlet/dsgps/model.py:130-163, mixed/dsgps/model.py:50-95): k updates
 *   h <- h + sigmoid(Wz c + bz) * tanh(Wc [sigmoid(Wr c + br) * h | mess_to | mess_from | prb] + bc),
 *   c = [h | Phi_to(h) | Phi_from(h) | prb], Dirichlet rows <- d_h0 rows; mixed plans: Neumann rows <-
 *   update_neumann([h | Phi_neumann(h) | prb | normal]) (d_normals required),
 * starting from d_h0 (the encoder state).  Tiled plans.  d_weights: psignn_dsgps_weights_size(mixed) floats
 * (layout in csrc/dsgps_tile.hip, built by engine.pack_dsgps); d_work: 4 * N * 10 floats (ws::DsgpsWork).
 * psignn_dsgps_step_p: a single update with all node tensors in plan order. */
int64_t psignn_dsgps_weights_size(int mixed);
int psignn_dsgps_forward(const psignn_plan_t* plan, const float* d_weights, int k, const float* d_h0, const float* d_prb,
                         const float* d_normals, float* d_out, float* d_work, void* stream);
int psignn_dsgps_step_p(const psignn_plan_t* plan, const float* d_weights, const float* d_h, const float* d_h0,
                        const float* d_prb, const float* d_normals, float* d_out, void* stream);
/* Backward of one DS-GPS update h' = step(h) (both families, caller's numbering): what loss.backward() runs per unrolled
 * update of ModelDSGPS.forward (dirichlet/dsgps/model.py:72-89, mixed/dsgps/model.py:72-93; training_class.py of those
 * directories).  d_w: cotangent on h'.  d_out_h = w^T dh'/dh (the Dirichlet rows' share goes to H_0: it is d_w on those
 * rows); d_grad: psignn_dsgps_grad_size(mixed) floats = the f_theta gradient layout (phi_to / phi_from slots, mixed: also
 * phi_neumann | update_neumann; psignn_param_grad_size(mixed, 1)) followed by [Wz (10 x (30+P)) | bz | Wr | br | Wc | bc].
 * d_phi_weights: those modules in the f_theta weight layout (psignn_weights_size(mixed, 1) floats; only their blocks are
 * read); d_gate_weights: [Wz | bz | Wr | br | Wc | bc] as nn.Linear stores them.  d_normals: mixed plans.
 * d_work: psignn_dsgps_step_backward_workspace_floats(plan) floats (ws::dsgps_bw_work). */
int64_t psignn_dsgps_grad_size(int mixed);
int64_t psignn_dsgps_step_backward_workspace_floats(const psignn_plan_t* plan);
int psignn_dsgps_step_backward(const psignn_plan_t* plan, const float* d_phi_weights, const float* d_gate_weights,
                               const float* d_h, const float* d_prb, const float* d_normals, const float* d_w, float* d_grad,
                               float* d_out_h, float* d_work, void* stream);

/* DSS, the Deep Statistical Solver baseline (dirichlet/dss/model.py:97-120): k updates with per-step weights
 *   h <- h + alpha * Psi_t([h | Phi_to_t(h) | Phi_from_t(h) | b'_norm]),  H_0 = 0,
 * on a tiled plan created with edge_attr = (0, 0, a_ij_norm) (the scalar edge feature of DSS).  d_weights:
 * psignn_dss_weights_size(k) floats (layout in csrc/dss_tile.hip, built by engine.pack_dss); d_work: N * 23 floats (ws::DssWork). */
int64_t psignn_dss_weights_size(int k);
int psignn_dss_forward(const psignn_plan_t* plan, const float* d_weights, int k, float alpha, const float* d_bprime_norm,
                       float* d_out, float* d_work, void* stream);
/* update t alone, state and b'_norm in plan order (the per-step loop of DeepStatisticalSolver.forward, model.py:77-93) */
int psignn_dss_step_p(const psignn_plan_t* plan, const float* d_weights, int t, float alpha, const float* d_h,
                      const float* d_bprime_norm_p, float* d_out, void* stream);
/* Backward of one DSS update h' = h + alpha Psi_t([h | Phi_to_t(h) | Phi_from_t(h) | b'_norm]) (caller's numbering): what
 * loss.backward() runs per update of DeepStatisticalSolver.forward (dirichlet/dss/model.py:75-83).  d_weights_t: update t's
 * modules in the f_theta weight layout with three node inputs (psignn_weights_size(1, 1)-style layout without Neumann blocks:
 * phi W1 padded to (10, 23) with the edge-feature weight in column 22, Psi in the update slots; engine.pack_dss_train builds
 * it).  d_grad: psignn_dss_grad_size() floats in that layout; d_out_h = w^T dh'/dh.
 * d_work: psignn_dss_step_backward_workspace_floats(plan) floats (ws::dss_bw_work). */
int64_t psignn_dss_grad_size(void);
int64_t psignn_dss_step_backward_workspace_floats(const psignn_plan_t* plan);
int psignn_dss_step_backward(const psignn_plan_t* plan, const float* d_weights_t, float alpha, const float* d_h,
                             const float* d_bprime_norm, const float* d_w, float* d_grad, float* d_out_h, float* d_work,
                             void* stream);

/* ------------------------------------------------------------------------------------------
 * Small dense pieces around the solve.
 * replaces: Encoder / Decoder MLPs (model.py:370-392), residual_loss SpMV (model.py:157-167).
 * ------------------------------------------------------------------------------------------ */
/* out (N, dout) = W2 relu(W1 x + b1) + b2 with W1 (hid,din), W2 (dout,hid); din,hid,dout <= 16 */
int psignn_mlp2(const float* d_x, int64_t n, int din, int hid, int dout,
                const float* d_w1, const float* d_b1, const float* d_w2, const float* d_b2,
                float* d_out, void* stream);
/* d_out (N) = A u - y  (A incl. diagonal). */
int psignn_residual(const psignn_plan_t* plan, const float* d_u, const float* d_y, float* d_out, void* stream);

/* ------------------------------------------------------------------------------------------
 * On-device Broyden root-find of g(x) = f(x) - x.
 * replaces: broyden(f, x0, threshold, eps, stop_mode="rel", ls=False)
 *           (dirichlet/psignn/utilities/solver.py:116-207) with matvec/rmatvec (:96-114) and the
 *           two .item() syncs per iteration (:162-163).
 * The inverse-Jacobian factors are stored U:(thr, N*d), V:(thr, N*d) row-contiguous.
 * ------------------------------------------------------------------------------------------ */
typedef struct psignn_broyden psignn_broyden_t;

typedef struct {
  int32_t nstep;        /* index of the lowest-residual iterate ("nstep" of the reference dict) */
  int32_t n_iter;       /* iterations executed (= len(xest_trace) - 1) */
  int32_t prot_break;
  int32_t stop_reason;  /* 0 threshold, 1 rel<eps, 2 plateau, 3 protective break */
  double lowest;        /* lowest rel residual */
  double lowest_abs;
} psignn_solve_info_t;

/* keep_trace != 0 stores every iterate ((thr+1) * N * d floats) for xest_trace. */
int psignn_broyden_create(psignn_broyden_t** out, const psignn_plan_t* plan, int threshold, int keep_trace);
void psignn_broyden_destroy(psignn_broyden_t* s);
/* stop_mode of the following solves: 0 = "rel" (default; all reference call sites), 1 = "abs" (utilities/solver.py:116,140,174):
 * objective, lowest-iterate tracking and the protective-break factor (1e6 instead of 1e3) follow it. */
int psignn_broyden_set_stop_mode(psignn_broyden_t* solver, int abs_mode);
size_t psignn_broyden_bytes(const psignn_broyden_t* s);

/* Solve; synchronous at the end (the result must be complete when it returns).  The host polls the
 * device-side status every `poll_every` iterations (<=0: default 8).
 * d_result: (N, d) lowest-residual iterate.  h_rel_trace / h_abs_trace: host arrays of
 * `threshold` doubles (may be NULL). */
int psignn_broyden_solve(psignn_broyden_t* s, const float* d_weights, int n_layers,
                         const float* d_h_initial, const float* d_prb, const float* d_normals,
                         double eps, int poll_every, float* d_result, psignn_solve_info_t* h_info,
                         double* h_rel_trace, double* h_abs_trace, void* stream);
/* Batched solve of n independent meshes (one GPU's share of a batch: BASELINE configs[3], 8 x 50k-node meshes): the meshes
 * iterate in lockstep and every per-iteration pass (fused f step, dots, reduce + stop tests, axpy, final) is ONE launch over
 * all of them; each mesh keeps its own status block, traces and stop test, and its result is bit-identical to
 * psignn_broyden_solve with the same solver on that mesh alone.  solvers[i] was created from mesh i's plan (tiled plans of ONE
 * family -- all dirichlet or all mixed, d_normals then holds the unit normals, else NULL --, one threshold and vector-size class
 * for the shard: psignn_broyden_batchable; otherwise PSIGNN_EINVAL).
 * replaces: the reference's one-union-Batch-per-device DataParallel call (dirichlet/psignn/main.py:106, mixed/psignn/main.py:106,
 *           dirichlet/psignn/test/test_func.py:68-120) for independent per-mesh solves.
 * Arrays of n device / host pointers; h_rel_trace[i] / h_abs_trace[i]: `threshold` doubles each (arrays may be NULL). */
/* Solver for mesh `plan` that will be used inside psignn_broyden_solve_batch together with others: shard_elems = sum of
 * N * d over the shard.  Its reduction shapes (vector width, split of the sweeps over the stored pairs) are sized for the
 * shard, not for the single mesh; psignn_broyden_solve on such a solver gives the same bits as the batched solve. */
int psignn_broyden_create_for_batch(psignn_broyden_t** out, const psignn_plan_t* plan, int threshold, int keep_trace,
                                    int64_t shard_elems);
int psignn_broyden_solve_batch(int n, psignn_broyden_t** solvers, const float* d_weights, int n_layers,
                               const float* const* d_h_initial, const float* const* d_prb, const float* const* d_normals,
                               double eps, int poll_every, float* const* d_results, psignn_solve_info_t* h_infos,
                               double* const* h_rel_trace, double* const* h_abs_trace, void* stream);
/* 1 when psignn_broyden_solve_batch takes these solvers together (tiled plans of one boundary-condition family, one size class),
 * else 0 -- asked on the host before a shard is handed over, so that "not batchable" is a decision and not an error code.
 * replaces: nothing in the reference (its DataParallel call takes any list of graphs as one union batch,
 *           dirichlet/psignn/main.py:106; mixed/psignn/main.py:106). */
int psignn_broyden_batchable(int n, psignn_broyden_t* const* solvers);
/* Adjoint fixed point y = J_f(h*)^T y + grad with the same Broyden machinery, the VJP kernel as the map, y_0 = 0.
 * replaces: the backward hook of DeepEquilibrium.forward (dirichlet/psignn/model.py:210-223), i.e.
 *           solver(lambda y: autograd.grad(new_H, H, y) + grad, zeros, bw_thres, bw_tol).
 * All tensors in the caller's numbering.  Multi-layer dirichlet blocks: the layer states h_1..h_{L-1} at h* are evaluated once
 * per solve into memory the solver owns (allocated on the first such solve, freed with the solver); every iteration then runs
 * the L backward layers only. */
int psignn_broyden_solve_adjoint(psignn_broyden_t* s, const float* d_weights, int n_layers, const float* d_h_star,
                                 const float* d_prb, const float* d_normals, const float* d_grad, double eps,
                                 int poll_every, float* d_result, psignn_solve_info_t* h_info,
                                 double* h_rel_trace, double* h_abs_trace, void* stream);
/* The same adjoint solve with psignn_lin_vjp as the map: h* is the state `lin` was last built at (on the solver's plan; a
 * linearisation of another plan is refused).  d_grad and d_result in the caller's numbering.
 * replaces: the backward hook of DeepEquilibrium.forward (dirichlet/psignn/model.py:210-223), with the Jacobian at H* linearised once
 *           instead of re-derived by autograd in every solver step. */
int psignn_broyden_solve_adjoint_lin(psignn_broyden_t* s, const psignn_lin_t* lin, const float* d_weights, int n_layers,
                                     const float* d_grad, double eps, int poll_every, float* d_result,
                                     psignn_solve_info_t* h_info, double* h_rel_trace, double* h_abs_trace, void* stream);
/* Batched adjoint solve: the lockstep form of psignn_broyden_solve_adjoint_lin for the n meshes of one shard.  Per iteration ONE launch
 * per pass over all meshes: x_next, the batched transposed product of the stored linearisations (out_m = J_m^T y_m), the residual
 * (J^T y + grad) - y with its norm partials, and the update chain psignn_broyden_solve_batch issues; every mesh keeps its own status
 * block, traces and stop test (a mesh whose test has fired is skipped while the others go on).  For every mesh n_iter, nstep,
 * stop_reason, both traces and the result are bit-identical to psignn_broyden_solve_adjoint_lin with the same solver object on that
 * mesh alone.  solvers[i] was created from mesh i's plan with shard_elems (psignn_broyden_create_for_batch), lins[i] was made for
 * that plan and built at the mesh's h*; the lazy first-call work of psignn_lin_vjp runs per handle before the loop.  Single-layer
 * blocks.  A shard psignn_broyden_adjoint_batchable does not take is PSIGNN_EINVAL with nothing launched.
 * replaces: the R replicas of the reference's DataParallel training step (dirichlet/psignn/main.py:106, mixed/psignn/main.py:106), each
 *           running the backward hook of DeepEquilibrium.forward (dirichlet/psignn/model.py:210-223) as an independent fixed-point
 *           problem with its own Broyden matrix and stop test.
 * Arrays of n device / host pointers; d_grads[i], d_results[i] in the caller's numbering; h_rel_trace[i] / h_abs_trace[i]: `threshold`
 * doubles each (arrays may be NULL). */
int psignn_broyden_solve_adjoint_lin_batch(int n, psignn_broyden_t** solvers, const psignn_lin_t* const* lins, const float* d_weights,
                                           int n_layers, const float* const* d_grads, double eps, int poll_every,
                                           float* const* d_results, psignn_solve_info_t* h_infos, double* const* h_rel_trace,
                                           double* const* h_abs_trace, void* stream);
/* 1 when psignn_broyden_solve_adjoint_lin_batch takes these solvers and linearisations together: all that psignn_broyden_batchable
 * asks of the solvers, and every lins[i] was made for solvers[i]'s plan, has been built, and holds a form the batched product takes
 * (dirichlet handles; mixed handles only with the Neumann rows stored, psignn_lin_create_opts(.., 1)).  0 otherwise, also for NULL
 * arguments -- a host-side question, asked before a shard is handed over.
 * replaces: nothing in the reference (its DataParallel replicas, dirichlet/psignn/main.py:106, each run their own backward hook,
 *           dirichlet/psignn/model.py:210-223, whatever the meshes are). */
int psignn_broyden_adjoint_batchable(int n, psignn_broyden_t* const* solvers, const psignn_lin_t* const* lins);
/* Copy iterate i (0..n_iter) of the last solve to d_dst (needs keep_trace). */
int psignn_broyden_get_iterate(const psignn_broyden_t* s, int i, float* d_dst, void* stream);
/* Copy stored rank-one pair j (0 .. pairs stored - 1) of the last solve to d_dst: which = 0 -> U_j, 1 -> V_j; which = 2 -> the current
 * `update` vector (solver.py:136,192; j ignored).  Caller's numbering.
 * replaces: reading Us[..., j] / VTs[:, j] of broyden() (utilities/solver.py:134-135, written at :190-191); the reference keeps them
 *           as locals of the solver call -- here they stay on the device between solves.  Used by the parity tests to check
 *           the Broyden recurrences of every update form on the device's own state. */
int psignn_broyden_get_pair(const psignn_broyden_t* s, int j, int which, float* d_dst, void* stream);

/* Generic low-rank machinery for user-supplied f (Python callables): the solver-API drop-in
 * `broyden(f, x0, threshold, eps)` drives these from the host with one f call per iteration.
 *   step_begin: x_new = x + update                      -> returns pointer-free: writes d_x_new
 *   step_end:   given fx = f(x_new): residual norms, stop test, rank-1 update, next update. */
int psignn_broyden_ext_begin(psignn_broyden_t* s, const float* d_x0, const float* d_fx0, void* stream);
int psignn_broyden_ext_next_x(psignn_broyden_t* s, float* d_x_new, void* stream);
/* Line search of `broyden(..., ls=True)` (line_search / scalar_search_armijo, utilities/solver.py:20-94): the host
 * evaluates phi(s) = |g(x + s * update)|^2 at trial points (ext_trial_x writes x + s * update, no state change) and
 * commits the accepted step length with ext_scale_step (update <- s * update) before ext_next_x / ext_update. */
int psignn_broyden_ext_trial_x(psignn_broyden_t* s, double step, float* d_x_trial, void* stream);
int psignn_broyden_ext_scale_step(psignn_broyden_t* s, double step, void* stream);
/* returns 1 in *h_done when the stop test fired (synchronous read of the status). */
int psignn_broyden_ext_update(psignn_broyden_t* s, const float* d_fx_new, double eps, int* h_done, void* stream);
int psignn_broyden_ext_finish(psignn_broyden_t* s, float* d_result, psignn_solve_info_t* h_info,
                              double* h_rel_trace, double* h_abs_trace, void* stream);
/* Same, for a problem that is not tied to a mesh plan (any vector length). */
int psignn_broyden_create_n(psignn_broyden_t** out, int64_t n_elems, int seq_len, int threshold, int keep_trace);
/* One constructor for every solver kind, with the element type of the stored rank-one pairs.  plan != NULL: a solver for that mesh
 * (n_elems, seq_len: 0 or the plan's N * d, d; shard_elems as in psignn_broyden_create_for_batch); plan == NULL: a vector of n_elems
 * elements, as psignn_broyden_create_n.  history = 0: fp32 pairs -- the same solver as create / create_n / create_for_batch give;
 * history = 1: bf16 pairs, each rounded to nearest even when it is written, every quantity derived from a new pair taking its rounded
 * value (so B = -I + sum U_j V_j^T over the stored bf16 values), arithmetic, iterate and update in fp32: half the pair memory and
 * half the bytes each iteration streams; always the unfolded three-sweep update, not batchable (psignn_broyden_batchable = 0).
 * Other values: PSIGNN_EINVAL.  psignn_broyden_get_pair returns a bf16 pair widened (exactly) to fp32.
 * replaces: broyden(f, x0, threshold, eps) (dirichlet/psignn/utilities/solver.py:116-207) with its Us / VTs (:134-135, written at
 *           :190-191) stored in bfloat16 instead of the iterate's dtype. */
int psignn_broyden_create_opts(psignn_broyden_t** out, const psignn_plan_t* plan, int64_t n_elems, int seq_len, int threshold,
                               int keep_trace, int64_t shard_elems, int history);

/* ------------------------------------------------------------------------------------------
 * Picard iteration and Anderson acceleration: the vector work, norms, stop tests and the small bordered solve on the
 * device; the caller evaluates f between the calls (the HIP GNN block, or any function of device tensors).
 * replaces: forward_iteration (dirichlet/psignn/utilities/solver.py:301-341) and anderson (:215-293, m = 2, lam = 1e-4,
 *           beta = 1 at every call site) -- their torch.linalg.norm / .item() per iteration, bmm, linalg.solve and the
 *           alpha @ F mixing.
 * n_elems = N * d.  m: history length of Anderson (1..8; Picard ignores it).  threshold: the reference's `threshold`.
 * keep_trace != 0 stores every iterate (threshold + 2 vectors) for xest_trace.  Device status block: after the stop test
 * has fired every later call is a no-op, so a caller may run a few iterations ahead of psignn_fpiter_poll.
 * ------------------------------------------------------------------------------------------ */
typedef struct psignn_fpiter psignn_fpiter_t;
int psignn_fpiter_create(psignn_fpiter_t** out, int64_t n_elems, int m, int threshold, int keep_trace);
void psignn_fpiter_destroy(psignn_fpiter_t* s);
size_t psignn_fpiter_bytes(const psignn_fpiter_t* s);
int psignn_fpiter_poll(psignn_fpiter_t* s, int* h_done, void* stream);     /* synchronous read of the done flag */
/* Picard: begin(z0); then repeat { current_x -> x ; fx = f(x) ; update(fx) }: abs = |x - fx|, rel = abs / |fx| appended
 * to the traces, stop when rel <= eps or after threshold + 1 evaluations, the current iterate becomes fx.
 * h_done may be NULL (no host read). */
int psignn_picard_begin(psignn_fpiter_t* s, const float* d_x0, void* stream);
int psignn_picard_current_x(psignn_fpiter_t* s, float* d_x, void* stream);
int psignn_picard_update(psignn_fpiter_t* s, const float* d_fx, double eps, int* h_done, void* stream);
/* Anderson: begin(x0, f(x0), f(f(x0))); then for k = 2 .. threshold - 1 { next_x -> x_k ; fx = f(x_k) ; update(fx) }.
 * next_x: Gram matrix of the residual history, alpha from the bordered system [[0, 1^T], [1, G G^T + lam I]], x_k =
 * beta sum alpha_i F_i + (1 - beta) sum alpha_i X_i.  update: rel = |fx - x_k| / (1e-5 + |fx|), traces, lowest iterate
 * by stop_mode (stop_abs: 0 "rel", 1 "abs"), stop when the objective < eps. */
int psignn_anderson_begin(psignn_fpiter_t* s, const float* d_x0, const float* d_f0, const float* d_f1, double lam, double beta,
                          int stop_abs, void* stream);
int psignn_anderson_next_x(psignn_fpiter_t* s, float* d_x_new, void* stream);
int psignn_anderson_update(psignn_fpiter_t* s, const float* d_fx_new, double eps, int* h_done, void* stream);
/* Result (Picard: the last iterate, nstep = ite, lowest = last rel; Anderson: the lowest iterate, nstep = its loop index),
 * traces (n_iter entries each; arrays of threshold + 2 doubles) and, for Anderson, per loop iteration the loop index of the
 * lowest iterate so far (h_low_idx, threshold + 2 int32, may be NULL).  Synchronous. */
int psignn_fpiter_finish(psignn_fpiter_t* s, float* d_result, psignn_solve_info_t* h_info, double* h_rel_trace,
                         double* h_abs_trace, int32_t* h_low_idx, void* stream);
/* Iterate i of the last run (keep_trace): Picard z_i; Anderson the trial point of loop index i (i >= 2). */
int psignn_fpiter_get_iterate(const psignn_fpiter_t* s, int i, float* d_dst, void* stream);
/* A handle for one mesh of a shard that psignn_anderson_solve_batch / psignn_picard_solve_batch will solve together: as
 * psignn_fpiter_create, except that the vector width (4 or 16 floats per lane) follows shard_elems = the sum of N * d over the shard
 * (>= n_elems) and not n_elems, so that all handles of a shard share one; blocks, partials and the row stride stay the mesh's own.  It
 * also holds the rows the lockstep solves keep per mesh (the map's value, its plan-order inputs).  The stepwise calls above work on such
 * a handle and give the bits of the lockstep solve.
 * replaces: the per-graph state of forward_iteration / anderson (dirichlet/psignn/utilities/solver.py:301-341, :215-293) when the
 *           graphs of one device's share of a batch (dirichlet/psignn/main.py:106) are solved side by side. */
int psignn_fpiter_create_for_batch(psignn_fpiter_t** out, int64_t n_elems, int m, int threshold, int keep_trace, int64_t shard_elems);
/* 1 when the lockstep solves below take these handles and plans together: n >= 1, all plans tiled and of one boundary-condition family,
 * handles[i] made by psignn_fpiter_create_for_batch for the length of plans[i], one vector width, one m, one threshold and
 * keep_trace == 0.  0 otherwise, also for NULL arguments -- asked on the host before a shard is handed over, so that "not batchable" is
 * a decision and not an error code.
 * replaces: nothing in the reference (its DataParallel call takes any list of graphs, dirichlet/psignn/main.py:106;
 *           mixed/psignn/main.py:106). */
int psignn_fpiter_batchable(int n, psignn_fpiter_t* const* handles, const psignn_plan_t* const* plans);
/* Lockstep Anderson acceleration of the n meshes of one shard with the HIP GNN block as the map: x0 = h_initial, f0 = f(x0),
 * f1 = f(f0), then the loop k = 2 .. threshold - 1, every pass -- Gram partials, bordered solve, mix, f, norms, stop test, gated copy of
 * the lowest iterate -- ONE launch over all meshes.  Every mesh keeps its own status block, traces, stop test and lowest iterate; a mesh
 * that has stopped is skipped by every later launch.  The all-done word is read every poll_every passes (<= 0: 8); results do not depend
 * on it.  Per mesh the result, info, traces and h_low_idx are those of psignn_anderson_begin / next_x / update / psignn_fpiter_finish
 * on the same handle around psignn_f_forward_p, bit for bit.  Tensors in the caller's numbering, as psignn_broyden_solve_batch takes
 * them (d_normals: NULL for dirichlet shards).  A shard psignn_fpiter_batchable refuses, n_layers != 1 and m < 2 are PSIGNN_EINVAL with
 * nothing launched.
 * replaces: anderson(f, x0, m, lam, threshold, eps, stop_mode, beta) (dirichlet/psignn/utilities/solver.py:215-293) called once per
 *           graph by DeepEquilibrium.forward (dirichlet/psignn/model.py:189, test/model_psignn.py:226) for the graphs of one device's
 *           share of a batch (dirichlet/psignn/main.py:106, test/test_func.py:68-120).
 * Arrays of n device / host pointers; h_rel_trace[i] / h_abs_trace[i]: threshold + 2 doubles, h_low_idx[i]: threshold + 2 int32 (arrays
 * may be NULL). */
int psignn_anderson_solve_batch(int n, psignn_fpiter_t** handles, const psignn_plan_t* const* plans, const float* d_weights,
                                int n_layers, const float* const* d_h_initial, const float* const* d_prb,
                                const float* const* d_normals, double lam, double beta, int stop_abs, double eps, int poll_every,
                                float* const* d_results, psignn_solve_info_t* h_infos, double* const* h_rel_trace,
                                double* const* h_abs_trace, int32_t* const* h_low_idx, void* stream);
/* The same for the Picard iteration z <- f(z) from z0 = h_initial: per pass f, norms, the gated move to the next iterate and the stop
 * test, one launch each over the shard, up to threshold + 1 evaluations; per mesh the bits of psignn_picard_begin / current_x / update /
 * psignn_fpiter_finish on the same handle.
 * replaces: forward_iteration(f, z0, eps, threshold) (dirichlet/psignn/utilities/solver.py:301-341) called once per graph
 *           (--solver forward_iteration) for the graphs of one device's share of a batch (dirichlet/psignn/main.py:106). */
int psignn_picard_solve_batch(int n, psignn_fpiter_t** handles, const psignn_plan_t* const* plans, const float* d_weights, int n_layers,
                              const float* const* d_h_initial, const float* const* d_prb, const float* const* d_normals, double eps,
                              int poll_every, float* const* d_results, psignn_solve_info_t* h_infos, double* const* h_rel_trace,
                              double* const* h_abs_trace, void* stream);

/* ------------------------------------------------------------------------------------------
 * GMRES on the device for the Newton-Krylov solver (BASELINE configs[4]: "Newton-Krylov JVP path").
 * replaces: nothing executable -- scipy.optimize.newton_krylov is imported at utilities/solver.py:6 and never called; with
 *           fp32 finite-difference products scipy's solver does not converge on this problem, the
 *           analytic JVP kernel (psignn_f_jvp_p) is the operator here.
 * The caller owns the basis d_basis: (m_max + 1) rows of `ld` floats (ld >= n_elems, a multiple of 4).  Per Arnoldi step j
 * it writes the raw operator product of basis row j into row j + 1 and calls psignn_gmres_step, which orthogonalises it
 * (classical Gram-Schmidt twice), updates the Hessenberg least-squares problem by Givens rotations and raises the device
 * stop flag once |residual| <= eta |b|.  Krylov operator: A v = product - shift * v (shift = 1 for A = J_f - I).
 * ------------------------------------------------------------------------------------------ */
typedef struct psignn_gmres psignn_gmres_t;
int psignn_gmres_create(psignn_gmres_t** out, int64_t n_elems, int64_t ld, int m_max, float* d_basis);
void psignn_gmres_destroy(psignn_gmres_t* s);
/* Device bytes the handle allocated itself (the caller's basis not counted): Hessenberg / Givens state and the dot partials, one row
 * per block of the vector kernels -- so two handles of one n_elems and m_max differ here exactly when their vector widths differ. */
size_t psignn_gmres_bytes(const psignn_gmres_t* s);
/* g = fx - x -> d_g (may be NULL), -g -> d_neg_g (may be NULL); h_norms[0] = |g|, h_norms[1] = |fx|.  Synchronous. */
int psignn_residual_norms(psignn_gmres_t* s, const float* d_x, const float* d_fx, float* d_g, float* d_neg_g, double* h_norms,
                          void* stream);
int psignn_gmres_begin(psignn_gmres_t* s, const float* d_b, void* stream);               /* basis row 0 = b / |b| */
int psignn_gmres_step(psignn_gmres_t* s, int j, double shift, double eta, int* h_done /* may be NULL */, void* stream);
/* d_dst = d_base + scale * z, z = the least-squares solution over the first k steps (k <= 0: all completed; d_base may be
 * NULL).  h_info (may be NULL): [steps completed, |b|, |residual|].  d_dst may alias d_base. */
int psignn_gmres_solution(psignn_gmres_t* s, int k, const float* d_base, double scale, float* d_dst, double* h_info, void* stream);
int psignn_gmres_history(psignn_gmres_t* s, double* h_res /* m_max + 1 */, void* stream);
/* Steps of the current solve whose second Gram-Schmidt pass ran (the pass is conditional: Daniel-Gragg-Kaufman-Stewart test on
 * the device, |w'|^2 < 1/2 |w|^2; PSIGNN_GMRES_REORTH=always makes it unconditional). */
int psignn_gmres_reorth_count(psignn_gmres_t* s, int* h_count, void* stream);

/* ------------------------------------------------------------------------------------------
 * Restarted GMRES for the adjoint system of the implicit backward (opt-in; model config key bw_solver = "gmres").
 * replaces: the backward hook of DeepEquilibrium.forward (dirichlet/psignn/model.py:210-223), which solves the LINEAR system
 *           y = J_f(h*)^T y + grad with Broyden (bw_tol 1e-8 is below fp32 resolution: that solve always runs its whole budget and
 *           keeps 2 * bw_thres vectors).  Here: GMRES with restart length m = m_max of the handle, (m + 1) basis vectors, the same
 *           products.  A departure from the reference's algorithm, not from what it solves.
 * Per cycle, all on the stream: r = (J^T y + grad) - y and rel = |r| / (|J^T y + grad| + 1e-9) -- the Broyden solver's measure, so
 * eps means what bw_tol means --, then up to m Arnoldi steps on the raw products (classical Gram-Schmidt twice, second pass
 * conditional; Givens; shift 1) until the least-squares residual is <= eps / 2 * |J^T y + grad|, then y -= V z.  The first cycle
 * starts from y = 0 and spends no product on its residual.  The solve ends at a cycle's check on rel < eps (stop_reason 1), on
 * rel > 1/2 of the previous cycle's rel (2: stagnation at the working precision) or when max_products are spent (0; one product is
 * kept back for the last residual, so `lowest` is always a measured value).  The result is the iterate with the lowest rel.
 * Every reduction has a fixed shape: the same call gives the same bits, and poll_every (how often the host looks at the cycle flag;
 * <= 0: 8) changes neither bits nor counts.  Synchronous at the end.
 * h_rel_trace / h_abs_trace: one entry per cycle, host arrays of max_products / 2 + 3 doubles (may be NULL). */
typedef struct {
  int32_t products;     /* transposed products spent */
  int32_t cycles;       /* restart cycles begun = entries of the traces */
  int32_t stop_reason;  /* 0 budget, 1 rel < eps, 2 stagnation */
  int32_t n_reorth;     /* Arnoldi steps whose second Gram-Schmidt pass ran */
  double lowest;        /* rel of the returned iterate */
  double lowest_abs;    /* its |r| */
} psignn_gmres_adjoint_info_t;
/* Floats of d_work for a solve on `plan` with blocks of n_layers (operator scratch, iterate, best iterate, plan-order copies of the
 * inputs, the layer states of a multi-layer dirichlet block: ws::AdjWork); -1 on bad arguments.  (model.py:210-223: none of this is kept there.) */
int64_t psignn_gmres_adjoint_workspace_floats(const psignn_plan_t* plan, int n_layers);
/* The solve with the VJP kernels as the map (model.py:210-223, autograd.grad(new_H, H, y) per step there): tiled plans run in plan
 * order on psignn_f_vjp_p (multi-layer dirichlet blocks: the layer states once, then the backward layers per product), untiled plans
 * on psignn_f_vjp; both families, any n_layers -- the choice psignn_broyden_solve_adjoint makes.  The handle was created for
 * n_elems = N * d of the plan.  All tensors in the caller's numbering. */
int psignn_gmres_solve_adjoint(psignn_gmres_t* s, const psignn_plan_t* plan, const float* d_weights, int n_layers,
                               const float* d_h_star, const float* d_prb, const float* d_normals, const float* d_grad, double eps,
                               int max_products, int poll_every, float* d_work, float* d_result,
                               psignn_gmres_adjoint_info_t* h_info, double* h_rel_trace, double* h_abs_trace, void* stream);
/* The same with psignn_lin_vjp as the map (model.py:210-223 with the Jacobian at H* linearised once): h* is the state `lin` was last
 * built at; both families, lin_neumann = "stored" handles included.  d_work is sized for the linearisation's plan. */
int psignn_gmres_solve_adjoint_lin(psignn_gmres_t* s, const psignn_lin_t* lin, const float* d_weights, int n_layers,
                                   const float* d_grad, double eps, int max_products, int poll_every, float* d_work,
                                   float* d_result, psignn_gmres_adjoint_info_t* h_info, double* h_rel_trace, double* h_abs_trace,
                                   void* stream);
/* A GMRES handle that will be used inside psignn_gmres_solve_adjoint_lin_batch together with others: shard_elems = the sum of n_elems
 * over the shard (>= n_elems).  The vector width of its sweeps follows shard_elems by the rule psignn_gmres_create applies to n_elems,
 * so that all handles of a shard share one; everything else is psignn_gmres_create.  Its single solves
 * (psignn_gmres_solve_adjoint / _lin) use that width too, hence give the same bits as its batched ones.
 * replaces: nothing in the reference (dirichlet/psignn/main.py:106: its DataParallel replicas share no solver state;
 *           dirichlet/psignn/model.py:210-223 keeps none between calls). */
int psignn_gmres_create_for_batch(psignn_gmres_t** out, int64_t n_elems, int64_t ld, int m_max, float* d_basis, int64_t shard_elems);
/* 1 when psignn_gmres_solve_adjoint_lin_batch takes these handles and linearisations together: all handles have one vector width and
 * one restart length m_max, every lins[i] has been built and holds a form the batched transposed product takes (dirichlet handles;
 * mixed handles only with the Neumann rows stored, psignn_lin_create_opts(.., 1)), solvers[i] was made for the N * d of lins[i]'s plan,
 * all plans are of one boundary-condition family and no handle appears twice.  0 otherwise, also for NULL arguments -- a host-side
 * question, asked before a shard is handed over.
 * replaces: nothing in the reference (its DataParallel replicas, dirichlet/psignn/main.py:106, each run their own backward hook,
 *           dirichlet/psignn/model.py:210-223, whatever the meshes are). */
int psignn_gmres_adjoint_batchable(int n, psignn_gmres_t* const* solvers, const psignn_lin_t* const* lins);
/* Batched restarted GMRES: the lockstep form of psignn_gmres_solve_adjoint_lin for the n replicas of one shard.  The restart cycles
 * are aligned across the replicas and every pass is ONE launch over all of them (blockIdx.z = replica): the cycle's residual product
 * and each Arnoldi step's product through the batched transposed product of the stored linearisations, then begin / check / keep /
 * scale, the Gram-Schmidt passes, finish, back-solve and combine.  Every replica keeps its own cycle and solve state, step allowance,
 * stop tests and traces; one whose cycle or solve is over is skipped while the others go on.  Per cycle the host reads every replica's
 * done flag and step allowance once, and every poll_every steps (<= 0: 8) one all-cycles-over flag.  For every replica the result,
 * products, cycles, stop_reason, n_reorth, lowest, lowest_abs and both traces are bit-identical to psignn_gmres_solve_adjoint_lin with
 * the same handle on that replica alone, for any poll_every.  d_works[i]: psignn_gmres_adjoint_workspace_floats(plan_i, 1) floats.
 * Single-layer blocks.  A shard psignn_gmres_adjoint_batchable does not take is PSIGNN_EINVAL with nothing launched.
 * replaces: the R replicas of the reference's DataParallel training step (dirichlet/psignn/main.py:106, mixed/psignn/main.py:106), each
 *           running the backward hook of DeepEquilibrium.forward (dirichlet/psignn/model.py:210-223) as an independent linear system.
 * Arrays of n device / host pointers; d_grads[i], d_results[i] in the caller's numbering; h_rel_trace[i] / h_abs_trace[i]:
 * max_products / 2 + 3 doubles each (arrays may be NULL). */
int psignn_gmres_solve_adjoint_lin_batch(int n, psignn_gmres_t** solvers, const psignn_lin_t* const* lins, const float* d_weights,
                                         int n_layers, const float* const* d_grads, double eps, int max_products, int poll_every,
                                         float* const* d_works, float* const* d_results, psignn_gmres_adjoint_info_t* h_infos,
                                         double* const* h_rel_trace, double* const* h_abs_trace, void* stream);
/* Augmented restarts (LGMRES; Baker, Jessup, Manteuffel 2005) and a settable stall ratio for the restarted fp32 adjoint solve,
 * opt-in; the method is the one psignn_gmres64_solve_adjoint_opts below runs in float64 (stated in the header of
 * csrc/krylov_f64.hip), here with fp32 vectors.  A solve keeps the `augment` newest corrections dy / |dy| of its cycles in a ring and,
 * of the steps a cycle may take, spends the last ka = min(stored, augment, left - 1) on them: one product J^T zhat each, w = J^T zhat -
 * zhat, orthogonalised against the basis like a Krylov vector.  The ring is cleared at the start of every solve.  stall: the solve
 * ends at the head of a cycle c > 0 when !(rel <= stall * prev_rel); 0.5 is the rule of psignn_gmres_solve_adjoint, 1.0 stops only
 * when a cycle does not lower rel at all.  {0, 0.5} launches the kernels of the entry points without options, with their arguments,
 * and gives their bits.  The lockstep solve above takes no options.
 * replaces: nothing of the reference; options of the solve that stands for dirichlet/psignn/model.py:210-223. */
typedef struct {
  int32_t augment; /* corrections kept, 0 .. the handle's augment */
  double stall;    /* in (0, 1] */
} psignn_gmres_opts_t;
/* psignn_gmres_adjoint_info_t (unchanged) plus the augmentation steps of the solve (model.py:210-223 reports none of this). */
typedef struct {
  int32_t products, cycles, stop_reason, n_reorth;
  double lowest, lowest_abs;
  int32_t n_aug;
} psignn_gmres_info_t;
/* psignn_gmres_create with a caller-owned ring of (augment + 1) rows of ld floats beside the basis, 0 <= augment <= min(m_max - 1, 8)
 * (one slot more than a cycle reads, so that the cycle's correction is written while the kept ones are read).  shard_elems = 0: sized
 * for itself; otherwise psignn_gmres_create_for_batch's rule.  augment = 0 with a NULL ring is psignn_gmres_create / _create_for_batch;
 * d_ring is NULL exactly when augment is 0.
 * replaces: nothing kept between solves at dirichlet/psignn/model.py:210-223. */
int psignn_gmres_create_aug(psignn_gmres_t** out, int64_t n_elems, int64_t ld, int m_max, float* d_basis, int augment, float* d_ring,
                            int64_t shard_elems);
/* psignn_gmres_solve_adjoint with options: opts->augment above the handle's, or stall outside (0, 1] or NaN, is PSIGNN_EINVAL before
 * any launch.  Traces, poll_every, determinism, d_work and d_result as there.
 * replaces: the solve of dirichlet/psignn/model.py:210-223 (autograd.grad(new_H, H, y) per step there), by another method. */
int psignn_gmres_solve_adjoint_opts(psignn_gmres_t* s, const psignn_plan_t* plan, const float* d_weights, int n_layers,
                                    const float* d_h_star, const float* d_prb, const float* d_normals, const float* d_grad, double eps,
                                    int max_products, int poll_every, const psignn_gmres_opts_t* opts, float* d_work, float* d_result,
                                    psignn_gmres_info_t* h_info, double* h_rel_trace, double* h_abs_trace, void* stream);
/* psignn_gmres_solve_adjoint_lin with the same options, refused in the same way.
 * replaces: the solve of dirichlet/psignn/model.py:210-223 with the Jacobian at H* linearised once, by another method. */
int psignn_gmres_solve_adjoint_lin_opts(psignn_gmres_t* s, const psignn_lin_t* lin, const float* d_weights, int n_layers,
                                        const float* d_grad, double eps, int max_products, int poll_every,
                                        const psignn_gmres_opts_t* opts, float* d_work, float* d_result, psignn_gmres_info_t* h_info,
                                        double* h_rel_trace, double* h_abs_trace, void* stream);

/* ------------------------------------------------------------------------------------------
 * Reference solve of the discrete Poisson system A u = y on the device: Jacobi-preconditioned conjugate gradient in float64 on the
 * plan's own matrix structure (csrc/poisson_cg.hip).  The ground truth `sol` of the accuracy metric mse_loss(u, batch.sol), at any size.
 * replaces: the direct solve of the reference's dataset builder (dirichlet/dataset/extract_data.py: solve(a == L, u, bc), LU; mixed:
 *           mixed/dataset/extract_data.py) and this repository's host stand-in for it, data/hexmesh.py _solve (scipy spsolve).
 * Rows with node flag bit0 (Dirichlet) are fixed, x_i = y_i, and none of their entries is read; the free rows F solve the lifted system
 * A_FF x_F = b, b = y_F - A_FD y_D (the mixed family's Neumann rows are free rows).  The handle keeps its own float64 copy of the
 * values (a 64-row sliced ELL in the plan's canonical column order), made once from d_a_ij in edge_index order, float32 (widened
 * exactly) or float64; the plan is not needed after create.
 * A position (i, j) may be given more than once (edge_index may repeat a pair): A_ij is the SUM of the entries given for it, added in
 * edge-id order in float64.  The solve multiplies by those sums, and symmetry, sym_defect and max |a_ij| below are judged on them: v, v
 * against a single v is unsymmetric (2v != v); v/2, v/2 against a single v is symmetric.
 * create checks what conjugate gradients need and fails with PSIGNN_EINVAL otherwise: every free-free position has its transposed
 * position and max |A_ij - A_ji| <= 1e-6 * max |A_ij| (a symmetric input rounds symmetrically: a valid matrix without repeated positions
 * has defect 0; sums of differently split pieces may differ by their rounding), every free row has a diagonal (the sum of its self
 * loops) > 0, every value on a free row is finite -- the entries in Dirichlet columns included, the entries of Dirichlet rows not: those
 * are never read and may hold anything.  Synchronous.
 * ------------------------------------------------------------------------------------------ */
typedef struct psignn_cg psignn_cg_t;
typedef struct {
  int32_t n_iter;       /* iterations run */
  int32_t converged;    /* 1: |r| <= tol |b| was met; 0: max_iter spent, or p.Ap <= 0 met (the iterate before it is returned) */
  double rel;           /* |r| / |b| of the recurrence residual at the end */
  double true_rel;      /* |(y - A x)_F| / |b|, recomputed from the returned x */
  double b_norm;        /* |b|, the lifted right-hand side on F */
  double sym_defect;    /* max |A_ij - A_ji| over the free-free positions (repeated entries summed), measured at create */
} psignn_cg_info_t;
int psignn_cg_create(psignn_cg_t** out, const psignn_plan_t* plan, const void* d_a_ij /* (E) edge_index order */, int a_is_f64,
                     void* stream);
void psignn_cg_destroy(psignn_cg_t* s);
/* One solve, all vectors and scalars float64 on the device: per iteration q = A p (the direction p = z + beta p is formed inside this
 * launch), alpha, then x += alpha p, r -= alpha q, z = r / diag(A), then beta, the stop test |r| <= tol |b| and the trace entry: four
 * dependent launches, every reduction per-block partials summed by one block in a fixed order (no floating-point atomics: the same call
 * gives the same bits).  The host only reads a done flag every poll_every iterations (<= 0: 50); launches queued beyond the last
 * iteration return at once, so result, n_iter and trace do not depend on poll_every.  max_iter bounds the iterations (0: none).
 * |b| = 0 gives x_F = 0 with n_iter 0; a start that meets the test gives n_iter 0.  d_y: (N) float32 or float64.  d_x0: (N) start
 * (free rows are read) or NULL for zeros; may be d_sol.  d_sol: (N) float64, caller's numbering, holds the iterate during the solve.
 * h_res_trace: |r| / |b| after each iteration, entry 0 the start; n_iter + 1 entries are written.  Synchronous at the end. */
int psignn_cg_solve(psignn_cg_t* s, const void* d_y, int y_is_f64, const double* d_x0 /* NULL: zeros on free rows */, double tol,
                    int max_iter, int poll_every, double* d_sol /* (N) caller's numbering */, psignn_cg_info_t* h_info,
                    double* h_res_trace /* max_iter + 1 doubles or NULL */, void* stream);

/* ------------------------------------------------------------------------------------------
 * The forward path in float64 on the device: f, the encoder / decoder MLP and a Broyden solve with every scalar on the device
 * (csrc/fgnn_f64.hip, csrc/solver_f64.hip).  The float64 fixed point h* -- the truth the fp32 path is measured against -- at any size.
 * Default-width library only (latent width 10).  Nothing here shares arithmetic, weight layout or kernels with the fp32 entry points.
 * replaces: the reference run with --precision double (dirichlet/psignn/utilities/utils.py:28, passed to the reader in
 *           dirichlet/psignn/main.py:59-67), i.e. Function.forward (dirichlet/psignn/model.py:279-300, mixed/psignn/model.py:216-245),
 *           Encoder / Decoder (model.py:370-392) and broyden (utilities/solver.py:116-207) on float64 tensors.
 *
 * Weights: a flat float64 buffer of the deqdss.f.* tensors in state-dict order, each nn.Linear (out, in) row-major, no padding:
 *   laynorm.weight[10] laynorm.bias[10] alpha.0.weight[30+P] alpha.0.bias[1]
 *   per layer l: phi_to_list.l.mlp.mlp.{0.weight[10x23] 0.bias[10] 2.weight[10x10] 2.bias[10]}, phi_from_list.l.mlp.mlp.{same},
 *                update_list.l.mlp.{0.weight[10x(30+P)] 0.bias[10] 2.weight[10x10] 2.bias[10]}
 *   mixed only:  phi_neumann.mlp.mlp.{as phi_to}, update_neumann.mlp.{0.weight[10x(22+P)] 0.bias[10] 2.weight[10x10] 2.bias[10]}
 * with P = 2 (dirichlet) / 3 (mixed).  psignn_f64_weights_size is that length (1193 / 1924 for one layer; -1 for n_layers < 1) and
 * needs no GPU.
 * ------------------------------------------------------------------------------------------ */
typedef struct psignn_f64 psignn_f64_t;
int64_t psignn_f64_weights_size(int mixed, int n_layers);
/* The handle keeps its own float64 copy of edge_attr, made once from d_edge_attr ((E, 3) in edge_index order, float32 -- widened
 * exactly -- or float64) in the plan's canonical order: per node its out-edges and its in-edges, self loops removed, ascending edge id.
 * It borrows the plan, which must outlive it.  Synchronous. */
int psignn_f64_create(psignn_f64_t** out, const psignn_plan_t* plan, const void* d_edge_attr /* (E,3) edge_index order */,
                      int attr_is_f64, void* stream);
void psignn_f64_destroy(psignn_f64_t* f);
/* d_out = f(d_h; d_h_initial, d_prb, d_normals): SURVEY a1-a4 as the reference writes them -- per edge the whole message MLP on
 * [x_i | x_j | a_e], summed per node over the plan's CSC (Phi_to) / CSR (Phi_from, Phi_neumann); gate, update MLP, LayerNorm on the last
 * layer, Dirichlet rows from d_h_initial, the mixed family's Neumann rows replaced by update_neumann and its layer loop that never
 * reassigns h (the last layer on h is the block).  All arrays float64, caller's numbering, on tiled and untiled plans alike; any
 * degree, duplicate and one-directional edges.  One node per lane, no atomics: the same call gives the same bits.  d_out != d_h. */
int psignn_f64_forward(psignn_f64_t* f, const double* d_weights, int n_layers, const double* d_h, const double* d_h_initial,
                       const double* d_prb, const double* d_normals /* NULL for dirichlet plans */, double* d_out, void* stream);
/* out (n, dout) = W2 relu(W1 x + b1) + b2 in float64, W1 (hid, din), W2 (dout, hid); din, hid, dout <= 16.
 * replaces: Encoder / Decoder (model.py:370-392) on float64 tensors. */
int psignn_mlp2_f64(const double* d_x, int64_t n, int din, int hid, int dout, const double* d_w1, const double* d_b1,
                    const double* d_w2, const double* d_b2, double* d_out, void* stream);

/* Broyden in float64 (reference recurrences: ls = False, stop mode "rel"): rel = |g| / (|g + x| + 1e-9); the lowest-rel iterate is
 * kept; stops on rel < eps, on the 30-step plateau rule at 3 eps, on the protective break at rel_0 * 1e3 * d, or after `threshold`
 * steps; NaN -> 0 in the new pair; update = g - U (V^T g) with the new pair included.
 * replaces: broyden(f, x0, threshold, eps) on float64 tensors (utilities/solver.py:116-207, matvec / rmatvec :96-114).
 * create allocates the pairs in float64, 2 * threshold * N * d * 8 bytes, and fails with PSIGNN_ENOMEM and a message naming that size
 * when it cannot.  The solver borrows the map handle (and through it the plan). */
typedef struct psignn_broyden64 psignn_broyden64_t;
int psignn_broyden64_create(psignn_broyden64_t** out, psignn_f64_t* f, int threshold);
void psignn_broyden64_destroy(psignn_broyden64_t* s);
size_t psignn_broyden64_bytes(const psignn_broyden64_t* s);
/* One solve from d_x0.  Every dot, norm, coefficient and stop test is on the device; the update is the two-pass form (one sweep of the
 * stored pairs for the coefficients, one for the combinations); every reduction is per-block partials summed by one block in a fixed
 * order (no floating-point atomics: the same call gives the same bits).  The host reads one done flag every poll_every iterations
 * (<= 0: 16); launches queued past the last iteration return at once, so nothing in the result depends on poll_every.
 * d_result: (N, d) float64, the lowest-rel iterate (d_x0 itself if no step went below 1e8).  h_info: as psignn_broyden_solve
 * (nstep: the 1-based step of the lowest iterate; n_iter: steps taken).  h_rel_trace / h_abs_trace: `threshold` doubles each or NULL;
 * n_iter entries are written, entry i after step i + 1.  Synchronous at the end. */
int psignn_broyden64_solve(psignn_broyden64_t* s, const double* d_weights, int n_layers, const double* d_x0,
                           const double* d_h_initial, const double* d_prb, const double* d_normals, double eps, int poll_every,
                           double* d_result, psignn_solve_info_t* h_info, double* h_rel_trace, double* h_abs_trace, void* stream);

/* ------------------------------------------------------------------------------------------
 * J v and J^T w of f in float64 on the device (csrc/fgnn_f64_deriv.hip): the truth the fp32 derivative kernels are measured against,
 * at any size.  Same handle, weights, numbering and rules as psignn_f64_forward: gather form, one node per lane, per edge the
 * reference's whole message MLP differentiated line by line, ReLU' = 1 where the pre-activation is > 0, no atomics and a fixed
 * summation order (the same call gives the same bits).  Default-width library only.
 * d_work: psignn_f64_deriv_workspace_doubles(f, n_layers, transposed) doubles of the caller's (0 for J v of a single-layer or mixed
 * block: d_work may then be NULL); a smaller one is PSIGNN_ENOMEM with a message naming the bytes needed.  d_out aliases no input.
 * ------------------------------------------------------------------------------------------ */
int64_t psignn_f64_deriv_workspace_doubles(const psignn_f64_t* f, int n_layers, int transposed);
/* d_out = J_f(d_h) d_v.  One launch per layer gives the layer's value and tangent together (a multi-layer dirichlet chain stores no
 * states); Dirichlet rows get tangent 0, the mixed family's Neumann rows go through update_neumann, the LayerNorm tangent is on the
 * last layer only.
 * replaces: torch.autograd.functional.jvp through Function.forward in double precision (dirichlet/psignn/model.py:279-300,
 *           mixed/psignn/model.py:216-245); the reference itself only ever forms the transposed product. */
int psignn_f64_jvp(psignn_f64_t* f, const double* d_weights, int n_layers, const double* d_h, const double* d_h_initial,
                   const double* d_prb, const double* d_normals /* NULL for dirichlet plans */, const double* d_v, double* d_out,
                   double* d_work, int64_t work_doubles, void* stream);
/* d_out = J_f(d_h)^T d_w (+ d_add when not NULL: with d_add = grad this is the map y -> J^T y + grad of the adjoint system).  Two
 * gather passes, no scatter: per receiving node the node-local part and the cotangents of its message sums, then per sending node
 * the x_j side of the messages its neighbours received from it.  A multi-layer dirichlet block evaluates its L - 1 layer states at
 * d_h and runs the chain backwards.
 * replaces: autograd.grad(new_H, H, y) in double precision -- the backward hook's product, dirichlet/psignn/model.py:210-225
 *           (y = J^T y + grad), and jac_loss_estimate's, model.py:416-435. */
int psignn_f64_vjp(psignn_f64_t* f, const double* d_weights, int n_layers, const double* d_h, const double* d_h_initial,
                   const double* d_prb, const double* d_normals /* NULL for dirichlet plans */, const double* d_w,
                   const double* d_add /* NULL: none */, double* d_out, double* d_work, int64_t work_doubles, void* stream);

/* ------------------------------------------------------------------------------------------
 * The adjoint solve of the implicit backward in float64 on the device, y = J_f(h*)^T y + grad from y = 0: the solve the reference's
 * --precision switch also puts in double precision, and the truth the fp32 adjoint solves are measured against, at any size.
 * The map is psignn_f64_vjp with d_add = grad.  Default-width library only.  All arrays float64 in the caller's numbering;
 * d_work: the caller's psignn_f64_deriv_workspace_doubles(f, n_layers, 1) doubles (smaller: PSIGNN_ENOMEM naming the bytes).
 * ------------------------------------------------------------------------------------------ */
/* Broyden on the adjoint system: the recurrences, stop tests, traces and h_info of psignn_broyden64_solve, on the map above.  One
 * product per step; launches queued past the last step return at once (the product's too), so nothing depends on poll_every.
 * replaces: the backward hook in double precision, dirichlet/psignn/model.py:210-223:
 *           broyden(lambda y: autograd.grad(new_H, H, y) + grad, zeros_like(grad), threshold = bw_thres, eps = bw_tol). */
int psignn_broyden64_solve_adjoint(psignn_broyden64_t* s, const double* d_weights, int n_layers, const double* d_h_star,
                                   const double* d_h_initial, const double* d_prb, const double* d_normals, const double* d_grad,
                                   double eps, int poll_every, double* d_work, int64_t work_doubles, double* d_result,
                                   psignn_solve_info_t* h_info, double* h_rel_trace, double* h_abs_trace, void* stream);
/* Restarted GMRES(m) on the adjoint system (csrc/krylov_f64.hip): the cycle logic, stop reasons, counts and traces of
 * psignn_gmres_solve_adjoint above, with vectors, basis, coefficients and partials in float64 and every scalar on the device
 * (Givens part: csrc/gmres_dense.h).  create allocates the basis, (m + 1) * N * d * 8 bytes, and fails with PSIGNN_ENOMEM and a
 * message naming that size when it cannot.  The solver borrows the map handle (and through it the plan).
 * replaces: the linear system of the backward hook, dirichlet/psignn/model.py:210-223, which the reference solves with Broyden. */
typedef struct psignn_gmres64 psignn_gmres64_t;
int psignn_gmres64_create(psignn_gmres64_t** out, psignn_f64_t* f, int m /* restart length, 1 .. 4096 */);
void psignn_gmres64_destroy(psignn_gmres64_t* s);   /* (model.py:210-223: nothing is kept there between solves) */
size_t psignn_gmres64_bytes(const psignn_gmres64_t* s);   /* device bytes of the handle (model.py:210-223 has no counterpart) */
/* One solve.  eps bounds |f(y) - y| / (|f(y)| + 1e-9), f(y) = J^T y + grad, measured at the head of every cycle; the solve ends
 * there on rel < eps (stop_reason 1), on a cycle that did not halve rel (2) or when max_products are spent (0; one product is kept
 * back for the last residual).  d_result: the iterate with the lowest rel.  The host reads the solve state once per cycle and the
 * cycle flag every poll_every Arnoldi steps (<= 0: 8); kernels queued past the end of a cycle return at once, so neither bits nor
 * counts depend on poll_every; no floating-point atomics, fixed-shape reductions: the same call gives the same bits.
 * h_rel_trace / h_abs_trace: one entry per cycle, host arrays of max_products / 2 + 3 doubles (may be NULL).  Synchronous at the end.
 * replaces: the solve of dirichlet/psignn/model.py:210-223 in double precision, by another method. */
int psignn_gmres64_solve_adjoint(psignn_gmres64_t* s, const double* d_weights, int n_layers, const double* d_h_star,
                                 const double* d_h_initial, const double* d_prb, const double* d_normals, const double* d_grad,
                                 double eps, int max_products, int poll_every, double* d_work, int64_t work_doubles, double* d_result,
                                 psignn_gmres_adjoint_info_t* h_info, double* h_rel_trace, double* h_abs_trace, void* stream);
/* Augmented restarts (LGMRES; Baker, Jessup, Manteuffel 2005) and a settable stall ratio for the float64 GMRES, opt-in; the method
 * is stated in the header of csrc/krylov_f64.hip.  A solve keeps the `augment` newest corrections dy / |dy| of its cycles in a ring
 * and, of the steps a cycle may take, spends the last ka = min(stored, augment, left - 1) on them: one product A zhat each, w = A zhat
 * - shift zhat, orthogonalised against the basis like a Krylov vector.  The ring is cleared at the start of every solve.  stall: the
 * solve ends at the head of a cycle c > 0 when !(rel <= stall * prev_rel); 0.5 is the rule of psignn_gmres64_solve_adjoint, 1.0
 * stops only when a cycle does not lower rel at all.  {0, 0.5} launches the kernels of the entry points without options, with their
 * arguments, and gives their bits.
 * replaces: nothing of the reference; options of the solve that stands for dirichlet/psignn/model.py:210-223 in double precision. */
typedef struct {
  int32_t augment; /* corrections kept, 0 .. the handle's augment */
  double stall;    /* in (0, 1] */
} psignn_gmres64_opts_t;
/* psignn_gmres_adjoint_info_t (shared with the fp32 solver, unchanged) plus the augmentation steps of the solve. */
typedef struct {
  int32_t products, cycles, stop_reason, n_reorth;
  double lowest, lowest_abs;
  int32_t n_aug;
} psignn_gmres64_info_t;
/* psignn_gmres64_create with a ring of augment + 1 vectors of N * d doubles, 0 <= augment <= min(m - 1, 8) (one slot more than a
 * cycle reads, so that the cycle's correction is written while the kept ones are read); PSIGNN_ENOMEM names the ring's bytes when
 * they do not fit.  augment = 0 is psignn_gmres64_create.  psignn_gmres64_bytes counts the ring.
 * replaces: nothing kept between solves at dirichlet/psignn/model.py:210-223. */
int psignn_gmres64_create_aug(psignn_gmres64_t** out, psignn_f64_t* f, int m, int augment);
/* psignn_gmres64_solve_adjoint with options: opts->augment above the handle's, or stall outside (0, 1] or NaN, is PSIGNN_EINVAL
 * before any launch.  Traces, poll_every, determinism, d_work and d_result as there.
 * replaces: the solve of dirichlet/psignn/model.py:210-223 in double precision, by another method. */
int psignn_gmres64_solve_adjoint_opts(psignn_gmres64_t* s, const double* d_weights, int n_layers, const double* d_h_star,
                                      const double* d_h_initial, const double* d_prb, const double* d_normals, const double* d_grad,
                                      double eps, int max_products, int poll_every, const psignn_gmres64_opts_t* opts, double* d_work,
                                      int64_t work_doubles, double* d_result, psignn_gmres64_info_t* h_info, double* h_rel_trace,
                                      double* h_abs_trace, void* stream);

/* ------------------------------------------------------------------------------------------
 * Newton-Krylov in float64 on the device with a pseudo-transient shift (csrc/newton_f64.hip, csrc/krylov_f64.hip): a second float64
 * solver for the fixed point of f beside psignn_broyden64_solve, for the sizes at which Broyden stalls (I - J_f is indefinite there;
 * (1 + sigma) I - J_f with sigma large enough is not).  Default-width library only.  All arrays float64 in the caller's numbering.
 * replaces: the reference's --precision run of solver(f, x0, threshold, eps), dirichlet/psignn/model.py:189 (DeepEquilibrium.forward
 *           with config["solver"] = broyden / anderson on float64 tensors); the reference has no Newton method there.
 * ------------------------------------------------------------------------------------------ */
/* The shifted linear solve shift * delta = A delta + d_b from delta = 0, A = J_f(d_h) (transposed = 0, the product psignn_f64_jvp) or
 * J_f(d_h)^T (transposed = 1, psignn_f64_vjp); shift finite and >= 1.  The handle, basis, kernels and cycle structure of
 * psignn_gmres64_solve_adjoint, with three differences: the shift on the Hessenberg's diagonal is `shift`; the residual is
 * r = A delta + b - shift * delta; the measure is the linear one, rel = |r| / |b|, the solve ending at the head of a cycle on
 * rel <= eta (stop_reason 1), on a cycle that did not halve rel (2) or on a spent budget (0), a cycle on |g_{j+1}| <= eta * |b| (the
 * target of an inexact Newton step; the adjoint solve keeps its eps / 2).
 * b = 0: delta = 0, stop_reason 1, no product.  d_work: the larger of psignn_f64_deriv_workspace_doubles(f, n_layers, 0) and (.., 1)
 * doubles (smaller: PSIGNN_ENOMEM naming the bytes).  h_info, traces (rel: the linear measure), poll_every, determinism: as
 * psignn_gmres64_solve_adjoint.  d_result aliases neither d_h nor d_b.
 * replaces: nothing the reference runs -- the linear system of a Newton step on f(x) - x of dirichlet/psignn/model.py:189 in double
 *           precision (transposed = 0) and its dual (transposed = 1; shift 1: the system of model.py:210-223). */
int psignn_gmres64_solve_shifted(psignn_gmres64_t* s, const double* d_weights, int n_layers, const double* d_h,
                                 const double* d_h_initial, const double* d_prb, const double* d_normals, const double* d_b,
                                 double shift, int transposed, double eta, int max_products, int poll_every, double* d_work,
                                 int64_t work_doubles, double* d_result, psignn_gmres_adjoint_info_t* h_info, double* h_rel_trace,
                                 double* h_abs_trace, void* stream);
/* psignn_gmres64_solve_shifted with the options of psignn_gmres64_solve_adjoint_opts (an augmentation step forms A zhat - shift zhat
 * with this call's shift); refusals as there.
 * replaces: nothing the reference runs -- the linear system of a Newton step on f(x) - x of dirichlet/psignn/model.py:189 in double
 *           precision and its dual (shift 1: the system of model.py:210-223). */
int psignn_gmres64_solve_shifted_opts(psignn_gmres64_t* s, const double* d_weights, int n_layers, const double* d_h,
                                      const double* d_h_initial, const double* d_prb, const double* d_normals, const double* d_b,
                                      double shift, int transposed, double eta, int max_products, int poll_every,
                                      const psignn_gmres64_opts_t* opts, double* d_work, int64_t work_doubles, double* d_result,
                                      psignn_gmres64_info_t* h_info, double* h_rel_trace, double* h_abs_trace, void* stream);
/* The policy of the outer loop, host only (no device is touched): from the shift sigma of an attempted step and |g| before (g_old) and
 * at the trial point (g_new), *accept and the next shift.  Reject when g_new is not finite or g_new > growth * g_old: the next shift is
 * max(4 sigma, reject_floor).  Accept otherwise: sigma * g_new / g_old (switched evolution relaxation), exactly 0 when that is below
 * sigma_off.
 * replaces: nothing of the reference (dirichlet/psignn/model.py:189 calls solvers without a globalisation). */
double psignn_newton64_policy(double sigma, double g_old, double g_new, double growth, double reject_floor, double sigma_off,
                              int* accept);
/* Options of one solve.  The defaults the Python layer documents (sigma0 1, eta 1e-2, max_products 200, growth 2, reject_floor 1/16,
 * sigma_off 1e-8, max_rejects 8, threshold 50) are starting values from CPU runs on the stored fixtures, not tuned on a GPU. */
typedef struct {
  double eps;           /* the solve ends on rel = |g| / (|f(x)| + 1e-9) < eps, g = f(x) - x (Broyden's measure, stop mode "rel") */
  double sigma0;        /* the first shift is 1 + sigma0 */
  double eta;           /* tolerance of every linear solve, |r| <= eta |g| */
  double growth, reject_floor, sigma_off;   /* psignn_newton64_policy */
  int32_t threshold;    /* attempted steps at most */
  int32_t max_products; /* budget of every linear solve */
  int32_t max_rejects;  /* the solve ends after this many consecutive rejections */
  int32_t poll_every;   /* of the linear solves (<= 0: 8); changes neither bits nor counts */
} psignn_newton64_opts_t;
#define PSIGNN_NEWTON_THRESHOLD 0
#define PSIGNN_NEWTON_TOLERANCE 1
#define PSIGNN_NEWTON_REJECTS 2
typedef struct {
  int32_t nstep;        /* the accepted step of the lowest-rel state (0: the start) */
  int32_t n_iter;       /* attempted steps */
  int32_t n_accepted;   /* accepted steps */
  int32_t n_products;   /* products J v spent by all linear solves */
  int32_t n_feval;      /* evaluations of f: 1 + n_iter */
  int32_t stop_reason;  /* PSIGNN_NEWTON_* */
  double lowest, lowest_abs;
} psignn_newton64_info_t;
/* The handle owns a GMRES64 handle of restart length m, six state vectors of N * d doubles (x, f(x), g, the trial point, its f,
 * delta), block partials and the two norms the host reads per attempted step.  create fails with PSIGNN_ENOMEM and a message naming
 * the bytes when the basis or the vectors do not fit.  The solver borrows the map handle (and through it the plan).
 * replaces: nothing kept between calls at dirichlet/psignn/model.py:189. */
typedef struct psignn_newton64 psignn_newton64_t;
int psignn_newton64_create(psignn_newton64_t** out, psignn_f64_t* f, int m /* restart length, 1 .. 4096 */);
void psignn_newton64_destroy(psignn_newton64_t* s);   /* (model.py:189: nothing is kept there between solves) */
size_t psignn_newton64_bytes(const psignn_newton64_t* s);   /* device bytes of the handle (model.py:189 has no counterpart) */
/* One solve from d_x0.  Attempted step n: psignn_gmres64_solve_shifted on (1 + sigma_n) delta = J_f(x_n) delta + g(x_n), the trial
 * point x_n + delta, f there, |g| and |f| by per-block partials summed by one block in a fixed order (no atomics), read by the host,
 * which decides with psignn_newton64_policy: a rejected step leaves the state untouched bit for bit.  Ends on rel < eps, after
 * `threshold` attempted steps or `max_rejects` consecutive rejections.  d_result: the accepted state with the lowest rel (d_x0 when no
 * step went below it).  Host arrays, each may be NULL: h_rel_trace / h_abs_trace, threshold + 1 doubles, the start and every accepted
 * state; h_sigma_trace, threshold + 1 doubles, sigma_0 and the shift after every decision; h_trial_abs (|g| at every trial point),
 * h_accepted, h_krylov (products per attempted step), h_lin_stop (stop_reason of its linear solve): threshold entries each.
 * d_work as for psignn_gmres64_solve_shifted.  The same call gives the same bits, whatever poll_every.  Synchronous.
 * replaces: solver(lambda H: f(H, H_init, batch), H_init, threshold, eps) of dirichlet/psignn/model.py:189 in double precision, by
 *           another method. */
int psignn_newton64_solve(psignn_newton64_t* s, const double* d_weights, int n_layers, const double* d_x0, const double* d_h_initial,
                          const double* d_prb, const double* d_normals, const psignn_newton64_opts_t* opts, double* d_work,
                          int64_t work_doubles, double* d_result, psignn_newton64_info_t* h_info, double* h_rel_trace,
                          double* h_abs_trace, double* h_sigma_trace, double* h_trial_abs, int32_t* h_accepted, int32_t* h_krylov,
                          int32_t* h_lin_stop, void* stream);
/* psignn_newton64_create whose GMRES64 handle comes from psignn_gmres64_create_aug(m, augment), and psignn_newton64_solve whose
 * linear solves run psignn_gmres64_solve_shifted_opts with lin_opts (refused as there, before any launch).  lin_opts = {0, 0.5}
 * gives the bits of psignn_newton64_solve.
 * replaces: nothing kept between calls at dirichlet/psignn/model.py:189. */
int psignn_newton64_create_aug(psignn_newton64_t** out, psignn_f64_t* f, int m, int augment);
/* replaces: solver(lambda H: f(H, H_init, batch), H_init, threshold, eps) of dirichlet/psignn/model.py:189 in double precision, by
 *           another method. */
int psignn_newton64_solve_opts(psignn_newton64_t* s, const double* d_weights, int n_layers, const double* d_x0,
                               const double* d_h_initial, const double* d_prb, const double* d_normals,
                               const psignn_newton64_opts_t* opts, const psignn_gmres64_opts_t* lin_opts, double* d_work,
                               int64_t work_doubles, double* d_result, psignn_newton64_info_t* h_info, double* h_rel_trace,
                               double* h_abs_trace, double* h_sigma_trace, double* h_trial_abs, int32_t* h_accepted,
                               int32_t* h_krylov, int32_t* h_lin_stop, void* stream);

/* ------------------------------------------------------------------------------------------
 * Parameter gradients in float64 on the device (csrc/fgnn_f64_deriv.hip): the last link of loss.backward() in double precision, and
 * the truth the fp32 parameter-gradient kernels are measured against, at any size.  Same handle, weights, numbering and rules as
 * psignn_f64_vjp.  Every gradient is a sum over receiving nodes: one workgroup per chunk of psignn_f64_param_vjp_chunk_rows()
 * consecutive rows of the caller's numbering adds its rows' outer products in ascending row order (per edge list: edge position by
 * edge position) and writes one row of partials; the partial rows are then added in ascending order, 64 at a time, and those sums
 * in ascending order again.  No floating-point atomics, and a summation order that depends on the graph alone: the same call gives
 * the same bits, on tiled and untiled plans alike.  Default-width library only.
 * ------------------------------------------------------------------------------------------ */
/* Rows whose contributions one partial holds (the chunks start at row 0).
 * replaces: nothing of the reference (dirichlet/psignn/model.py:203-225 sums in autograd's order). */
int psignn_f64_param_vjp_chunk_rows(void);
/* Doubles of d_work for psignn_f64_param_vjp: psignn_f64_deriv_workspace_doubles(f, n_layers, 1) for the product J^T w, then
 * ceil(N / chunk_rows) * psignn_f64_weights_size(mixed, 1) for the partials.  -1 for a NULL handle or n_layers < 1.
 * replaces: autograd's saved tensors of dirichlet/psignn/model.py:203-225. */
int64_t psignn_f64_param_vjp_workspace_doubles(const psignn_f64_t* f, int n_layers);
/* d_grad (psignn_f64_weights_size(mixed, n_layers) doubles, the layout of d_weights, nothing padded): the gradient of
 * <d_w, f(d_h; d_h_initial)> with respect to every deqdss.f.* tensor.  d_out_h = J_f(d_h)^T d_w, the bits of psignn_f64_vjp.
 * d_out_init (may be NULL) = d_w^T df/dh_initial: the Dirichlet rows of the cotangent on every layer's output, summed over the
 * layers (single-layer block: d_w copied on the Dirichlet rows, 0 elsewhere).  Dirichlet family, n_layers > 1: the layer states at
 * d_h, then the chain backwards, layer k's gradient at (h_k, w_{k+1}); alpha.0.* accumulates over the layers from the last to the
 * first, laynorm.* comes from the last layer.  Mixed family: only the last layer's iteration reaches the output, so the earlier
 * layers' sections are exact zeros.  d_out_h aliases neither d_h nor d_w; a d_work smaller than the query is PSIGNN_ENOMEM with a
 * message naming the bytes.
 * replaces: loss.backward() into the deqdss.f.* parameters after the hook has swapped in the adjoint solution, in double precision
 *           (dirichlet/psignn/model.py:203-225; mixed/psignn/model.py likewise). */
int psignn_f64_param_vjp(psignn_f64_t* f, const double* d_weights, int n_layers, const double* d_h, const double* d_h_initial,
                         const double* d_prb, const double* d_normals /* NULL for dirichlet plans */, const double* d_w,
                         double* d_grad, double* d_out_h, double* d_out_init /* NULL: skip */, double* d_work, int64_t work_doubles,
                         void* stream);
/* Doubles of d_work for psignn_f64_vjp_backward: N * 10 * (2 + 2 * cw) for (loc, C) of J^T v and their tangents (cw = 2, mixed 3),
 * for a multi-layer dirichlet block N * 10 * (2 * (n_layers - 1) + 4) more (the layer states and their tangents, the ping-pongs of
 * the cotangent and of its tangent), then ceil(N / chunk_rows) * psignn_f64_weights_size(mixed, 1) for the partials.  -1 for a NULL
 * handle or n_layers < 1.
 * replaces: autograd's saved tensors of the double backward, dirichlet/psignn/model.py:416-435. */
int64_t psignn_f64_vjp_backward_workspace_doubles(const psignn_f64_t* f, int n_layers);
/* Backward of the VJP in float64: for psi = <d_gbar, J_f(d_h)^T d_v> with d_gbar constant, d_grad (psignn_f64_weights_size(mixed,
 * n_layers) doubles, the layout of d_weights) = d psi / d theta over every deqdss.f.* tensor, d_dh = d psi / d h, and d_jtv (may be
 * NULL) = J_f(d_h)^T d_v, the bits of psignn_f64_vjp.  psi is the derivative along d_gbar of <d_v, f(h)>, so every cotangent of the
 * reverse pass of psignn_f64_param_vjp travels with its tangent along dh = d_gbar: ReLU masks are constants of it, what remains is the
 * curvature of the gate and of LayerNorm.  The parameter sums follow the rule above (chunks of chunk_rows rows in ascending order,
 * partials added 64 at a time and then in ascending order, no floating-point atomics); a multi-layer dirichlet block is the chain
 * forward with (h_k, t_k), t_0 = d_gbar, and backwards with (w_k, dw_k), alpha.0.* accumulating from the last layer to the first; a
 * mixed block differentiates its last layer and leaves exact zeros in the earlier ones.  Both families, tiled or not, the caller's
 * numbering; the same call gives the same bits.  d_dh and d_jtv alias none of d_h, d_v, d_gbar or each other; a d_work smaller than
 * the query is PSIGNN_ENOMEM with a message naming the bytes.
 * replaces: what loss.backward() does with the Jacobian regulariser, in double precision -- jac_loss_estimate,
 *           dirichlet/psignn/model.py:416-435: autograd.grad(f0, z0, v, create_graph=True) and the backward of |v^T J|^2 / numel
 *           (mixed/psignn/model.py likewise). */
int psignn_f64_vjp_backward(psignn_f64_t* f, const double* d_weights, int n_layers, const double* d_h, const double* d_h_initial,
                            const double* d_prb, const double* d_normals /* NULL for dirichlet plans */, const double* d_v,
                            const double* d_gbar, double* d_grad, double* d_dh, double* d_jtv /* NULL: skip */, double* d_work,
                            int64_t work_doubles, void* stream);
/* psignn_f64_vjp_backward (the same launches, the same bits in every output it shares) and d_dinit (N, 10; may be NULL) = d psi /
 * d h_initial.  A multi-layer dirichlet block copies the Dirichlet rows of h_initial into every layer state h_1 .. h_{L-1}, and J_f is
 * evaluated at those states: d_dinit is the sum over them of the Dirichlet rows of the tangent of their cotangents.  Every other block
 * (single layer; mixed, whose loop never reassigns h) has a Jacobian that does not depend on h_initial: exact zeros.  This is the path by
 * which the Jacobian regulariser reaches the encoder.  d_dinit aliases none of the other arrays.
 * replaces: loss.backward() from jac_loss_estimate, dirichlet/psignn/model.py:416-435, into H_init = encoder(x) of
 *           DeepEquilibrium.forward (model.py:184-207), in double precision. */
int psignn_f64_vjp_backward_init(psignn_f64_t* f, const double* d_weights, int n_layers, const double* d_h, const double* d_h_initial,
                                 const double* d_prb, const double* d_normals /* NULL for dirichlet plans */, const double* d_v,
                                 const double* d_gbar, double* d_grad, double* d_dh, double* d_jtv /* NULL: skip */,
                                 double* d_dinit /* NULL: skip */, double* d_work, int64_t work_doubles, void* stream);
/* Doubles of d_work for psignn_mlp2_f64_backward: ceil(n / 128) * (hid * din + hid + dout * hid + dout); -1 for sizes out of range.
 * replaces: autograd's saved tensors of Encoder / Decoder, dirichlet/psignn/model.py:370-392. */
int64_t psignn_mlp2_f64_backward_workspace_doubles(int64_t n, int din, int hid, int dout);
/* Backward of psignn_mlp2_f64 (din, hid, dout <= 16, any n): from d_x (n, din) and d_gy (n, dout), d_gx (n, din; NULL: skip) and
 * d_gflat = [gW1 (hid, din) | gb1 | gW2 (dout, hid) | gb2] in float64.  Deterministic by the rule above: per-chunk partials of 128
 * rows, added in a fixed order.
 * replaces: autograd through Encoder / Decoder on float64 tensors, dirichlet/psignn/model.py:370-392. */
int psignn_mlp2_f64_backward(const double* d_x, const double* d_gy, int64_t n, int din, int hid, int dout, const double* d_w1,
                             const double* d_b1, const double* d_w2, double* d_gx, double* d_gflat, double* d_work,
                             int64_t work_doubles, void* stream);

/* ------------------------------------------------------------------------------------------
 * The losses of a training step in float64 on the device (csrc/poisson_cg.hip, beside the solve of the same system): the residual of the discrete Poisson system with its
 * transpose, and a mean-square error with its gradient -- with the entries above, every link of ModelDEQDSS._train_forward and of its
 * loss.backward() in double precision (engine.train_step64).  A = COO(edge_index, a_ij) including the diagonal; d_a_ij: the caller's
 * (E) float64 values in edge_index order (the plan's own copy is fp32 and is not read).  Caller's numbering, tiled and untiled plans
 * alike; any degree, duplicate and one-directional edges, nodes without a self loop.  No atomics, and sums whose order depends on
 * the graph or on the length alone: the same call gives the same bits.  Default-width library only.
 * ------------------------------------------------------------------------------------------ */
/* d_r (N) = A d_u - d_y: one row per lane over the plan's full CSR (columns ascending, equal columns by edge id), repeated positions
 * added entry after entry.  d_r aliases neither d_u nor d_y.
 * replaces: residual_loss before its mean, dirichlet/psignn/model.py:157-167 (index_add_ over edge_index), as ModelDEQDSS.forward
 *           calls it (model.py:58-99), on float64 tensors. */
int psignn_residual_f64(const psignn_plan_t* plan, const double* d_a_ij /* (E) edge_index order */, const double* d_u,
                        const double* d_y, double* d_r, void* stream);
/* d_out (N) = A^T d_r: per column its in-edges in the plan's CSC order (sender ascending, equal senders by edge id), then the diagonal
 * entries of its row of the full CSR -- psignn_residual_t in float64.  d_out must not alias d_r.
 * replaces: autograd through residual_loss, dirichlet/psignn/model.py:157-167, in the backward of model.py:58-99, on float64 tensors. */
int psignn_residual_t_f64(const psignn_plan_t* plan, const double* d_a_ij /* (E) edge_index order */, const double* d_r,
                          double* d_out, void* stream);
/* Elements whose squares one partial of psignn_mse_f64 holds (the chunks start at element 0).
 * replaces: nothing of the reference (F.mse_loss of dirichlet/psignn/model.py:58-99 and the mean of model.py:157-167 sum in torch's order). */
int psignn_mse_f64_chunk(void);
/* Doubles of d_work for psignn_mse_f64: ceil(n_elems / chunk), one partial per chunk; -1 for n_elems < 1.
 * replaces: nothing of the reference (model.py:157-167 and :58-99 keep no partial sums). */
int64_t psignn_mse_f64_workspace_doubles(int64_t n_elems);
/* *d_loss (one double on the device) = sum (d_a - d_b)^2 / scale_n over n_elems elements (d_b NULL: zeros), and, when d_grad is not
 * NULL, d_grad = 2 (d_a - d_b) / scale_n element by element.  One partial per chunk (thread t of the block adds elements t, t + 256,
 * ... of its chunk in ascending order, then the fixed block sum), then one block adds the partials in ascending stride order and
 * divides once.  n_elems < 1, scale_n <= 0 and a NULL d_a / d_loss are PSIGNN_EINVAL; d_grad, d_loss and d_work alias nothing else;
 * a d_work smaller than the query is PSIGNN_ENOMEM with a message naming the bytes.
 * replaces: torch.mean(residual ** 2), dirichlet/psignn/model.py:157-167, and the F.mse_loss terms of ModelDEQDSS.forward
 *           (model.py:58-99: encoder_loss, autoencoder_loss, mse_loss, mse_dirichlet) with their autograd, on float64 tensors. */
int psignn_mse_f64(const double* d_a, const double* d_b /* NULL: zeros */, int64_t n_elems, double scale_n /* the divisor */,
                   double* d_loss /* 1 double on the device */, double* d_grad /* NULL or n_elems */, double* d_work,
                   int64_t work_doubles, void* stream);

/* ------------------------------------------------------------------------------------------
 * Per-kernel timing with HIP events on the launch stream (used by bench.py for the roofline line;
 * replaces: the reference's only instrumentation, time.time() around the model call,
 * tests/special_geo/spec_geo_2.py:313-317).  Off by default.
 * ------------------------------------------------------------------------------------------ */
void psignn_prof_enable(int on);
int psignn_prof_collect(void);   /* sync + aggregate per kernel name; returns the number of names */
int psignn_prof_get(int i, char* name, int cap, int64_t* calls, double* total_ms);
/* The same plus the sum of the ALGORITHMIC bytes of those launches as the launch sites state them (stored pairs swept, kept
 * window, meshes of the shard: what actually ran) -- 0 for kernels that state none.  bench.py's roofline figures come from here. */
int psignn_prof_get2(int i, char* name, int cap, int64_t* calls, double* total_ms, int64_t* alg_bytes);
/* Launch i of the last collect, in launch order: kernel name, duration, stated algorithmic bytes.  name == NULL: returns the
 * number of launches.  (scripts/summarise_pmc.py lines rocprofv3's per-dispatch counters up with this log.) */
int psignn_prof_launch(int i, char* name, int cap, double* ms, int64_t* alg_bytes);
/* Diagnostics: d_buf = device array of n_tiles * 4 * 8 int64 (or NULL to switch off).  While set, every wave of the f tile
 * kernel stores shader-clock stamps at its phase boundaries (0 start, 1 stage 1 done, 2 past the barrier, 3 neighbour sums
 * done, 4 node update done, 5 stored) -- scripts/tile_phases.py turns them into a per-phase time budget. */
void psignn_prof_tile_stamps(void* d_buf);

#ifdef __cplusplus
}
#endif
#endif /* PSIGNN_HIP_H */
