// Derivatives of a multi-layer dirichlet block (n_layers = L > 1) as chains of single-layer derivatives (gfx950); the parameter
// VJP and the backward of the VJP of such blocks chain the same pieces in fgnn_pgrad.hip.
//
// Reference: Function.forward (dirichlet/psignn/model.py:279-300): alpha is shared by all layers, LayerNorm applies on the
// last layer only and the Dirichlet rows are overwritten with h_initial after EVERY layer:
//   h_0 = h,  h_{k+1} = F_k(h_k) = Dir(h_k + alpha * U_k(c_k(h_k))) for k < L-1,  f(h) = F_{L-1}(h_{L-1}) (with LayerNorm).
// With J_k = J_{F_k}(h_k) -- what the single-layer kernels compute at layer k's weights, LayerNorm switched off for k < L-1
// (the *_noln instantiations) --
//   JVP  t_0 = v, t_{k+1} = J_k t_k, result t_L;      VJP  w_L = w, w_k = J_k^T w_{k+1}, result w_0.
// The layer states h_1..h_{L-1} come from the forward layer kernels (k_f_tile_layer on tiled plans, k_project / k_node
// otherwise) with LayerNorm off, into the caller's layer workspace (psignn_f_layers_workspace_floats):
//   [ h_1 | ... | h_{L-1} | t_a | t_b ]   (N, 10) each; t_a / t_b carry the tangent / cotangent between layers.
// The entry points of f's derivatives do not take h_initial: the Dirichlet rows of h_1..h_{L-1} are taken from h's own
// Dirichlet rows.  That is exact wherever h's Dirichlet rows are h_initial's: every state f returns, h_initial itself, a
// fixed point -- each state a solver, the implicit backward or a training step differentiates at.
// Every step is a gather kernel or a tile kernel with a fixed walk order: no atomics, bitwise reproducible.
#include "fgnn_common.h"
#include "internal.h"

// Layer workspace (ws::LayerWork): the states h_1..h_{L-1}, the rows the chains carry between layers, and a single-layer view of
// the weights (psignn_f_layer_view).
static_assert(WLayout<3>::base_total(1, true) <= ws::LAYER_VIEW, "single-layer weight view");
extern "C" int64_t psignn_f_layers_workspace_floats(const psignn_plan_t* p, int n_layers) {
  if (!p || n_layers < 1 || n_layers > 64) return -1;
  return ws::layer_work(p->N, n_layers, p->mixed, nullptr).total;
}

// dst <- the single-layer weights of layer l in the base layout ([shared | layer l | mixed: phi_neumann, update_neumann, fold]):
// the weights the single-layer gather kernels of the backward of the VJP read (they address layer 0)
int psignn_f_layer_view(const psignn_plan* p, const float* W, int nl, int l, float* dst, hipStream_t st) {
  const size_t F = sizeof(float);
  if (p->mixed) {
    using L = WLayout<3>;
    HIP_TRY(hipMemcpyAsync(dst, W, L::SHARED_SZ * F, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(dst + L::layer(0), W + L::layer(l), L::LAYER_SZ * F, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(dst + L::phi_neu(1), W + L::phi_neu(nl), (size_t)(L::base_total(nl, true) - L::phi_neu(nl)) * F,
                           hipMemcpyDeviceToDevice, st));
  } else {
    using L = WLayout<2>;
    HIP_TRY(hipMemcpyAsync(dst, W, L::SHARED_SZ * F, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(dst + L::layer(0), W + L::layer(l), L::LAYER_SZ * F, hipMemcpyDeviceToDevice, st));
  }
  return PSIGNN_OK;
}

// dst[n] (+)= src[n] on the Dirichlet rows, 0 elsewhere (first: dst is overwritten): the h_initial cotangent of a block whose
// Dirichlet rows are copies of h_initial after every layer
__global__ __launch_bounds__(256) void k_dir_acc(int64_t N, const uint8_t* __restrict__ flags, const float* __restrict__ src,
                                                 float* __restrict__ dst, int first) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N * D) return;
  const float v = (flags[i / D] & FLAG_DIRICHLET) ? src[i] : 0.f;
  dst[i] = first ? v : dst[i] + v;
}
int psignn_f_dir_acc(const psignn_plan* p, const uint8_t* flags, const float* src, float* dst, int first, hipStream_t st) {
  PROF_BYTES(p->N * (1 + 40 + (first ? 40 : 80)));
  LAUNCH("k_dir_acc", st, (k_dir_acc<<<(unsigned)cdiv(p->N * D, 256), 256, 0, st>>>(p->N, flags, src, dst, first)));
  HIP_TRY(hipGetLastError());
  return PSIGNN_OK;
}
__global__ __launch_bounds__(256) void k_add_rows(int64_t n, const float* __restrict__ a, const float* __restrict__ b,
                                                  float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = a[i] + b[i];
}
int psignn_f_add_rows(const psignn_plan* p, const float* a, const float* b, float* out, hipStream_t st) {
  PROF_BYTES(p->N * D * 12);
  LAUNCH("k_add_rows", st, (k_add_rows<<<(unsigned)cdiv(p->N * D, 256), 256, 0, st>>>(p->N * D, a, b, out)));
  HIP_TRY(hipGetLastError());
  return PSIGNN_OK;
}

// h_1..h_{L-1} of the block at h into lw: tile kernels in plan order on tiled plans, unless gather (caller order, gather
// kernels; work: psignn_f_workspace_floats)
int psignn_f_layer_states(const psignn_plan* p, const float* W, int nl, const float* h, const float* prb, float* lw, float* work,
                          hipStream_t st, bool gather) {
  ARG_CHECK(p && !p->mixed && nl > 1 && lw, "layer states: multi-layer dirichlet blocks");
  const ws::LayerWork L = ws::layer_work(p->N, nl, false, lw);
  const float* cur = h;
  for (int l = 0; l + 1 < nl; ++l) {
    float* dst = L.state(l + 1);
    int rc = (p->tiled && !gather) ? psignn_f_tile_layer(p, W, nl, l, cur, h, prb, dst, st)
                                   : psignn_f_gather_layer(p, W, nl, l, cur, h, prb, nullptr, dst, work, st);
    if (rc) return rc;
    cur = dst;
  }
  return PSIGNN_OK;
}

// out = J_f(h)^T w from the layer states already in lw (psignn_f_layer_states); h, prb, w, out in the plan's numbering of the
// kernels that run (plan order on tiled plans)
int psignn_f_layers_vjp(const psignn_plan* p, const float* W, int nl, const float* h, const float* prb, const float* w, float* out,
                        float* work, float* lw, hipStream_t st) {
  const ws::LayerWork L = ws::layer_work(p->N, nl, false, lw);
  const float* cur = w;
  for (int k = nl - 1; k >= 0; --k) {
    const float* hk = k == 0 ? h : L.state(k);
    float* dst = k == 0 ? out : L.tb[(nl - 1 - k) & 1];
    int rc = p->tiled ? psignn_f_tile_vjp_layer(p, W, nl, k, hk, prb, cur, dst, work, nullptr, st)
                      : psignn_f_gather_vjp_layer(p, W, nl, k, hk, prb, cur, dst, work, st);
    if (rc) return rc;
    cur = dst;
  }
  return PSIGNN_OK;
}

// out = J_f(h) v, layer states in lw
int psignn_f_layers_jvp(const psignn_plan* p, const float* W, int nl, const float* h, const float* prb, const float* v, float* out,
                        float* work, float* lw, hipStream_t st) {
  const ws::LayerWork L = ws::layer_work(p->N, nl, false, lw);
  const float* cur = v;
  for (int k = 0; k < nl; ++k) {
    const float* hk = k == 0 ? h : L.state(k);
    float* dst = k == nl - 1 ? out : L.tb[k & 1];
    int rc = p->tiled ? psignn_f_tile_jvp_layer(p, W, nl, k, hk, prb, cur, dst, st)
                      : psignn_f_gather_layer(p, W, nl, k, hk, hk, prb, cur, dst, work, st);
    if (rc) return rc;
    cur = dst;
  }
  return PSIGNN_OK;
}

// Stateless forms (evaluate the layer states, then the chain).  lw: the layer workspace, which a caller of a multi-layer
// dirichlet derivative appends to the entry point's own workspace.
int psignn_f_layers_vjp_stateless(const psignn_plan* p, const float* W, int nl, const float* h, const float* prb, const float* w,
                                  float* out, float* work, float* lw, hipStream_t st) {
  int rc = psignn_f_layer_states(p, W, nl, h, prb, lw, work, st, false);
  return rc ? rc : psignn_f_layers_vjp(p, W, nl, h, prb, w, out, work, lw, st);
}
int psignn_f_layers_jvp_stateless(const psignn_plan* p, const float* W, int nl, const float* h, const float* prb, const float* v,
                                  float* out, float* work, float* lw, hipStream_t st) {
  int rc = psignn_f_layer_states(p, W, nl, h, prb, lw, work, st, false);
  return rc ? rc : psignn_f_layers_jvp(p, W, nl, h, prb, v, out, work, lw, st);
}

// ---- the operator of an adjoint solve (internal.h)
int AdjointOp::setup(const psignn_plan* p_, const float* W_, int nl_, const float* h_star, const float* prb_, const float* nrm_,
                     const float* grad_, ws::Adapter rows, float* fwork_, float* lwork_, hipStream_t st_) {
  p = p_; W = W_; nl = nl_; fwork = fwork_; lwork = lwork_; st = st_;
  tiled = p->tiled;
  layers = !p->mixed && nl > 1;
  h = h_star; prb = prb_; nrm = nrm_; grad = grad_;
  int rc;
  if (tiled) {
    if ((rc = psignn_to_plan(p, h_star, grad_, prb_, nrm_, rows, st))) return rc;
    h = rows.h; grad = rows.x; prb = rows.prb; nrm = rows.nrm;
  }
  return layers ? psignn_f_layer_states(p, W, nl, h, prb, lwork, fwork, st, false) : PSIGNN_OK;
}
int AdjointOp::operator()(const float* y, float* out) const {
  if (layers) return psignn_f_layers_vjp(p, W, nl, h, prb, y, out, fwork, lwork, st);
  return tiled ? psignn_f_vjp_p(p, W, nl, h, prb, nrm, y, out, fwork, st) : psignn_f_vjp(p, W, nl, h, prb, nrm, y, out, fwork, st);
}
