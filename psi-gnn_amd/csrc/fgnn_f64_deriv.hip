// J v and J^T w of f_theta in float64 (gfx950): the device's own statement of the float64 derivatives, at any size.
//
// replaces: autograd through Function.forward run in double precision -- what the reference's --precision switch selects for the
//           backward hook too (dirichlet/psignn/model.py:210-225: autograd.grad(new_H, H, y) inside the adjoint solve;
//           jac_loss_estimate model.py:416-435) on dirichlet/psignn/model.py:279-300 and mixed/psignn/model.py:216-245.
//
// The check on the fp32 derivative kernels, written like fgnn_f64.hip and for the same purpose: gather form, one node per lane,
// the CALLER's numbering, tiled and untiled plans alike; the flat state-dict weight buffer W64; per edge the whole message MLP of
// the reference, differentiated line by line; nothing shared with fgnn_tile_*.hip, fgnn_vjp.hip or WLayout; no atomics and a fixed
// summation order, so the same call gives the same bits.
//
// The node block -- the per-edge pieces, the node's forward with or without a tangent, LayerNorm, the node's reverse -- is
// f64_node.h's, stated once; the kernels here keep what is theirs: the loads, the stores and the LDS rounds.
//
// J v: one launch per layer gives the layer's value and its tangent together (k_f64_jvp_layer, f64_node.h), so a multi-layer
// dirichlet chain stores no states.
// J^T w: two gather passes, no scatter.  An edge (r, c) sits once in r's CSR list and once in c's CSC list with the same attribute
// row, so what a scatter would add to the sending node is gathered there from the receiving nodes' records:
//   pass A (k_f64_vjp_node), per receiving node n: the node's forward again, w_n back through LayerNorm, gate and update (or
//          update_neumann) -- the shared forward and reverse pieces --, the node-local part of the result -- the x_i side of its own edges' messages included -- and the
//          cotangents of its message sums C[n] = {c_to, c_from (, c_neu)}, zero on Dirichlet rows;
//   pass B (k_f64_vjp_edge), per sending node m: over m's CSR entries the x_j side of Phi_to at the neighbour with the neighbour's
//          c_to, over m's CSC entries the x_j side of Phi_from with c_from (Neumann neighbours: Phi_neumann with c_neu); every ReLU
//          mask recomputed from h.  Optionally + a vector to add, which makes the map of the adjoint system y -> J^T y + grad one call.
// Every kernel takes the done flag of a solver (NULL: none) and returns at once when it is set: psignn_f64_vjp_gated is the product of
// the float64 adjoint solves (solver_f64.hip, krylov_f64.hip), whose launches queued past the end of a solve or cycle change nothing.
// The weight layout W64, the map handle psignn_f64 and the family dispatch F64_FAMILY are those of fgnn_f64.hip: both files take
// them from f64_common.h.
#include "f64_common.h"
#include "f64_node.h"
#include <math.h>
#include <type_traits>

// ---------------------------------------------------------------------------------------------
// J^T w, pass A: per receiving node.  loc (N, D): the node-local part; C (N, CW): {c_to, c_from (, c_neu)}, CW = 2 D / 3 D.
// ---------------------------------------------------------------------------------------------
template <int P, bool MIXED>
__global__ __launch_bounds__(256) void k_f64_vjp_node(int64_t N, const double* __restrict__ W, int lofs, int nofs, int apply_ln,
                                                      const int32_t* __restrict__ csr_ptr, const int32_t* __restrict__ csr_nbr,
                                                      const double* __restrict__ csr_attr, const int32_t* __restrict__ csc_ptr,
                                                      const int32_t* __restrict__ csc_nbr, const double* __restrict__ csc_attr,
                                                      const uint8_t* __restrict__ flags, const double* __restrict__ h,
                                                      const double* __restrict__ prb, const double* __restrict__ nrm,
                                                      const double* __restrict__ w, double* __restrict__ loc, double* __restrict__ C,
                                                      const int32_t* __restrict__ done) {
  using L = W64<P>;
  constexpr int CW = MIXED ? 3 * D : 2 * D;
  if (done && *done) return;
  const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  const uint8_t fl = flags[n];
  double gx[D], c[3 * D];
#pragma unroll
  for (int k = 0; k < D; ++k) gx[k] = 0.0;
#pragma unroll
  for (int k = 0; k < 3 * D; ++k) c[k] = 0.0;
  if (!(fl & FLAG_DIRICHLET)) {   // a Dirichlet row is h_initial's: nothing flows back through it
    double x[D], gy[D];
    d64_row(h, n, x);
    d64_row(w, n, gy);
    const int32_t rb = csr_ptr[n], re = csr_ptr[n + 1], cb = csc_ptr[n], ce = csc_ptr[n + 1];
    // The node's forward again, then back, one kind of row per branch.  The record (yhat: d64_ln_back's by-product) is declared here
    // and shared by both branches, and the branch body is a lambda, not a helper template: either other form spills in <3, true>.
    double cat[L::CAT], rp[D], sv[D], y[D], yhat[D], g[D], q[D], al, dal, gal;
    unsigned mask;
    auto back = [&](auto kind) __attribute__((always_inline)) {
      constexpr bool NEU = decltype(kind)::value;
      d64_node_fwd<P, false, NEU>(W, lofs, nofs, n, x, nullptr, h, nullptr, csr_ptr, csr_nbr, csr_attr, csc_ptr, csc_nbr, csc_attr, prb,
                                  nrm, cat, nullptr, al, dal, mask, rp, nullptr, sv, nullptr, y, nullptr);
      if (apply_ln) d64_ln_back(W + L::LN_G, y, gy, yhat);
      d64_node_back_q<P, NEU>(W, lofs, nofs, mask, al, sv, gy, gal, g, q);
      d64_node_back_c<P, NEU>(W, lofs, nofs, gal, q, gy, c, gx);
      d64_node_back_xi<P, NEU>(W, lofs, nofs, x, h, rb, re, cb, ce, csr_nbr, csr_attr, csc_nbr, csc_attr, c, gx);
    };
    if (MIXED && (fl & FLAG_NEUMANN))
      back(std::true_type{});
    else
      back(std::false_type{});
  }
#pragma unroll
  for (int k = 0; k < D; ++k) loc[n * D + k] = gx[k];
#pragma unroll
  for (int k = 0; k < CW; ++k) C[n * CW + k] = c[k];
}

// ---------------------------------------------------------------------------------------------
// J^T w, pass B: per sending node m.  out[m] = loc[m] + sum over m's CSR entries (m -> u: u receives Phi_to from m)
//                + sum over m's CSC entries (u -> m: u receives Phi_from, or Phi_neumann, from m) (+ add[m]).
// Dirichlet neighbours hold zero cotangents and are passed over; of a Neumann neighbour only c_neu is non-zero.
// ---------------------------------------------------------------------------------------------
template <bool MIXED>
__global__ __launch_bounds__(256) void k_f64_vjp_edge(int64_t N, const double* __restrict__ W, int lofs, int nofs,
                                                      const int32_t* __restrict__ csr_ptr, const int32_t* __restrict__ csr_nbr,
                                                      const double* __restrict__ csr_attr, const int32_t* __restrict__ csc_ptr,
                                                      const int32_t* __restrict__ csc_nbr, const double* __restrict__ csc_attr,
                                                      const uint8_t* __restrict__ flags, const double* __restrict__ h,
                                                      const double* __restrict__ loc, const double* __restrict__ C,
                                                      const double* __restrict__ add, double* __restrict__ out,
                                                      const int32_t* __restrict__ done) {
  using L = W64<2>;
  constexpr int CW = MIXED ? 3 * D : 2 * D;
  if (done && *done) return;
  const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= N) return;
  double x[D], g[D];
  d64_row(h, m, x);
  d64_row(loc, m, g);
  for (int32_t i = csr_ptr[m]; i < csr_ptr[m + 1]; ++i) {
    const int64_t u = csr_nbr[i];
    const uint8_t fu = flags[u];
    if (fu & FLAG_DIRICHLET) continue;
    if (MIXED && (fu & FLAG_NEUMANN)) continue;   // a Neumann row has no Phi_to
    double xu[D], a[3], c[D];
    d64_row(h, u, xu);
#pragma unroll
    for (int k = 0; k < 3; ++k) a[k] = csr_attr[3 * (int64_t)i + k];
#pragma unroll
    for (int k = 0; k < D; ++k) c[k] = C[u * CW + k];
    d64_msg_vjp_xj(W + lofs, xu, x, a, c, g);
  }
  for (int32_t i = csc_ptr[m]; i < csc_ptr[m + 1]; ++i) {
    const int64_t u = csc_nbr[i];
    const uint8_t fu = flags[u];
    if (fu & FLAG_DIRICHLET) continue;
    const bool neu = MIXED && (fu & FLAG_NEUMANN);
    double xu[D], a[3], c[D];
    d64_row(h, u, xu);
#pragma unroll
    for (int k = 0; k < 3; ++k) a[k] = csc_attr[3 * (int64_t)i + k];
#pragma unroll
    for (int k = 0; k < D; ++k) c[k] = C[u * CW + (neu ? 2 * D : D) + k];
    d64_msg_vjp_xj(W + (neu ? nofs : lofs + L::PHI_SZ), xu, x, a, c, g);
  }
#pragma unroll
  for (int k = 0; k < D; ++k) out[m * D + k] = add ? g[k] + add[m * D + k] : g[k];
}

// ---------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------
// one layer's value (out_h, may be NULL) and, with v, its tangent (out_v)
static void jvp_launch(const psignn_f64* f, const double* W, int nl, int l, int apply_ln, const double* h, const double* v,
                       const double* h0, const double* prb, const double* nrm, double* out_h, double* out_v, const int32_t* done,
                       hipStream_t st) {
  const psignn_plan* p = f->p;
  const unsigned g = (unsigned)cdiv(p->N, 256);
  // algorithmic bytes: both edge lists once (neighbour id, 3 attributes, the neighbour's row and tangent row), per node its rows
  PROF_BYTES(2 * p->Ep * (4 + 24 + (v ? 16 : 8) * D) + p->N * ((v ? 32 : 16) * D + 8 * (p->mixed ? 3 : 2) + 17));
  if (v)
    F64_FAMILY(p->mixed, LAUNCH("k_f64_jvp_layer", st,
                                (k_f64_jvp_layer<P, MIXED, true><<<g, 256, 0, st>>>(p->N, W, L::layer(l), L::layer(nl), apply_ln,
                                                                                  F64_EDGES(f), h, v, h0, prb, nrm, out_h, out_v, done))));
  else
    F64_FAMILY(p->mixed, LAUNCH("k_f64_state_layer", st,
                                (k_f64_jvp_layer<P, MIXED, false><<<g, 256, 0, st>>>(p->N, W, L::layer(l), L::layer(nl), apply_ln,
                                                                                   F64_EDGES(f), h, nullptr, h0, prb, nrm, out_h,
                                                                                   nullptr, done))));
}

// pass B of one layer: out = loc + the x_j sides gathered from C (+ add)
static void vjp_edge_launch(const psignn_f64* f, const double* W, int nl, int l, const double* h, const double* loc, const double* C,
                            const double* add, double* out, const int32_t* done, hipStream_t st) {
  const psignn_plan* p = f->p;
  // both edge lists once (neighbour id and flag, 3 attributes, the neighbour's row and its cotangent), per node h, loc, out (, add)
  PROF_BYTES(2 * p->Ep * (4 + 1 + 24 + 16 * D) + p->N * (8 * 3 * D + (add ? 8 * D : 0) + 8));
  F64_FAMILY(p->mixed, LAUNCH("k_f64_vjp_edge", st,
                              (k_f64_vjp_edge<MIXED><<<(unsigned)cdiv(p->N, 256), 256, 0, st>>>(p->N, W, L::layer(l), L::layer(nl),
                                                                                              F64_EDGES(f), h, loc, C, add, out, done))));
}

// both passes of one layer: out = J_l(h)^T w (+ add)
static void vjp_launch(const psignn_f64* f, const double* W, int nl, int l, int apply_ln, const double* h, const double* prb,
                       const double* nrm, const double* w, double* loc, double* C, const double* add, double* out, const int32_t* done,
                       hipStream_t st) {
  const psignn_plan* p = f->p;
  const int cw = p->mixed ? 3 * D : 2 * D;
  PROF_BYTES(2 * p->Ep * (4 + 24 + 8 * D) + p->N * (8 * (3 * D + cw) + 8 * (p->mixed ? 3 : 2) + 17));
  F64_FAMILY(p->mixed, LAUNCH("k_f64_vjp_node", st,
                              (k_f64_vjp_node<P, MIXED><<<(unsigned)cdiv(p->N, 256), 256, 0, st>>>(
                                  p->N, W, L::layer(l), L::layer(nl), apply_ln, F64_EDGES(f), h, prb, nrm, w, loc, C, done))));
  vjp_edge_launch(f, W, nl, l, h, loc, C, add, out, done, st);
}

// Only a multi-layer dirichlet block is a chain: the mixed loop never reassigns h, so its last layer on h is the block.
static inline bool f64_chain(const psignn_f64* f, int nl) { return !f->p->mixed && nl > 1; }

// A block backwards.  A chain: the states h_1 .. h_{L-1} at h (t: with their tangents), then layer(l, end, h_l, t_l, w_{l+1}, dst)
// for l = L-1 .. 0, which leaves w_l = J_l^T w_{l+1} in dst: the ping-pong pp for the inner layers, out for the last step
// (end: l = 0).  Any other block: the one step, layer nl - 1 at h, straight into out; states, tans and pp are not touched.
template <class Layer>
static void f64_walk_back(const psignn_f64* f, const double* W, int nl, const double* h, const double* t, const double* h0,
                          const double* prb, double* states, double* tans, const double* w, double* pp, double* out,
                          const int32_t* done, hipStream_t st, Layer layer) {
  const int64_t row = f->p->N * D;
  const int first = f64_chain(f, nl) ? 0 : nl - 1;
  const double *ch = h, *ct = t;
  for (int l = first; l + 1 < nl; ++l) {
    jvp_launch(f, W, nl, l, 0, ch, ct, h0, prb, nullptr, states + l * row, t ? tans + l * row : nullptr, done, st);
    ch = states + l * row;
    if (t) ct = tans + l * row;
  }
  for (int l = nl - 1; l >= first; --l) {
    double* dst = l == first ? out : pp + (l & 1) * row;
    layer(l, l == first, l == first ? h : states + (l - 1) * row, l == first || !t ? t : tans + (l - 1) * row, w, dst);
    w = dst;
  }
}

extern "C" int64_t psignn_f64_deriv_workspace_doubles(const psignn_f64_t* f, int n_layers, int transposed) {
  if (!f || n_layers < 1) return -1;
  const int64_t row = f->p->N * D;
  const bool chain = f64_chain(f, n_layers);
  if (!transposed) return chain ? 4 * row : 0;                                          // value and tangent ping-pong
  return row * (1 + (f->p->mixed ? 3 : 2)) + (chain ? row * (n_layers - 1 + 2) : 0);   // loc, C; the states, cotangent ping-pong
}

static int work_check(const char* who, int64_t need, const double* work, int64_t have) {
  if (need > 0 && (!work || have < need)) {
    psignn_set_error("%s: the workspace holds %lld doubles, %lld are needed (%lld bytes)", who, (long long)(work ? have : 0),
                     (long long)need, (long long)need * 8);
    return PSIGNN_ENOMEM;
  }
  return PSIGNN_OK;
}

// The product with the flag of a solver (internal.h): every launch returns at once when *done is set (NULL: no flag).
int psignn_f64_jvp_gated(psignn_f64_t* f, const double* W, int nl, const double* h, const double* h0, const double* prb,
                         const double* nrm, const double* v, double* out, double* work, int64_t work_doubles, const int32_t* done,
                         hipStream_t st) {
  ARG_CHECK(f && W && h && h0 && prb && v && out, "NULL argument");
  ARG_CHECK(nl >= 1 && nl <= 64, "n_layers out of range");
  ARG_CHECK(!f->p->mixed || nrm, "mixed plan needs unit normals");
  ARG_CHECK(out != h && out != v, "out must not alias h or v");
  const int rc = work_check("psignn_f64_jvp", psignn_f64_deriv_workspace_doubles(f, nl, 0), work, work_doubles);
  if (rc) return rc;
  if (f->p->N == 0) return PSIGNN_OK;
  if (!f64_chain(f, nl)) {
    jvp_launch(f, W, nl, nl - 1, 1, h, v, h0, prb, nrm, nullptr, out, done, st);
  } else {
    const int64_t row = f->p->N * D;
    const double *ch = h, *cv = v;
    for (int l = 0; l < nl; ++l) {
      const bool last = l == nl - 1;
      double* dh = last ? nullptr : work + (l & 1) * row;
      double* dv = last ? out : work + (2 + (l & 1)) * row;
      jvp_launch(f, W, nl, l, last, ch, cv, h0, prb, nrm, dh, dv, done, st);
      ch = dh;
      cv = dv;
    }
  }
  HIP_TRY(hipGetLastError());
  return PSIGNN_OK;
}

extern "C" int psignn_f64_jvp(psignn_f64_t* f, const double* W, int nl, const double* h, const double* h0, const double* prb,
                              const double* nrm, const double* v, double* out, double* work, int64_t work_doubles, void* stream) {
  return psignn_f64_jvp_gated(f, W, nl, h, h0, prb, nrm, v, out, work, work_doubles, nullptr, (hipStream_t)stream);
}

// The transposed product with the flag of a solver, likewise.
int psignn_f64_vjp_gated(psignn_f64_t* f, const double* W, int nl, const double* h, const double* h0, const double* prb,
                         const double* nrm, const double* w, const double* add, double* out, double* work, int64_t work_doubles,
                         const int32_t* done, hipStream_t st) {
  ARG_CHECK(f && W && h && h0 && prb && w && out && work, "NULL argument");
  ARG_CHECK(nl >= 1 && nl <= 64, "n_layers out of range");
  ARG_CHECK(!f->p->mixed || nrm, "mixed plan needs unit normals");
  ARG_CHECK(out != h && out != w && out != add, "out must not alias h, w or add");
  const int rc = work_check("psignn_f64_vjp", psignn_f64_deriv_workspace_doubles(f, nl, 1), work, work_doubles);
  if (rc) return rc;
  if (f->p->N == 0) return PSIGNN_OK;
  const int64_t row = f->p->N * D;
  const bool chain = f64_chain(f, nl);
  double *loc = work, *C = work + row, *states = chain ? work + 3 * row : nullptr, *pp = chain ? work + (3 + nl - 1) * row : nullptr;
  f64_walk_back(f, W, nl, h, nullptr, h0, prb, states, nullptr, w, pp, out, done, st,
                [&](int l, bool end, const double* hl, const double*, const double* wl, double* dst) {
                  vjp_launch(f, W, nl, l, l == nl - 1, hl, prb, nrm, wl, loc, C, end ? add : nullptr, dst, done, st);
                });
  HIP_TRY(hipGetLastError());
  return PSIGNN_OK;
}

extern "C" int psignn_f64_vjp(psignn_f64_t* f, const double* W, int nl, const double* h, const double* h0, const double* prb,
                              const double* nrm, const double* w, const double* add, double* out, double* work,
                              int64_t work_doubles, void* stream) {
  return psignn_f64_vjp_gated(f, W, nl, h, h0, prb, nrm, w, add, out, work, work_doubles, nullptr, (hipStream_t)stream);
}

// =============================================================================================
// Parameter gradients in float64: the gradient of <w, f_theta(h; h_initial)> with respect to every deqdss.f.* tensor, in the flat
// layout of W64, and the backward of the encoder / decoder MLP.
//
// replaces: what loss.backward() leaves in the deqdss.f.* parameters once the hook has swapped in the adjoint solution
//           (dirichlet/psignn/model.py:203-225, mixed likewise), run in double precision; autograd through Encoder / Decoder
//           (model.py:370-392) on float64 tensors.
//
// Every parameter's gradient is a sum over RECEIVING nodes of outer products A (x) B, so nothing is scattered and nothing is added
// atomically.  One workgroup owns PG_ROWS consecutive rows of the caller's numbering (a chunk), one row per lane:
//   * the lane recomputes its node as pass A of J^T w does and keeps the cotangents of the gate, the update and the message sums;
//   * in rounds, every lane writes the two factors of one kind of outer product to its LDS row (Dirichlet rows, rows past the end
//     and rows the module does not act on: zeros), and after a barrier every thread, owning a few (o, k) entries of the module's
//     weight and bias, walks the PG_ROWS rows in ascending order.  Node rounds: update W1 + gate, update W2 + LayerNorm,
//     update_neumann; then per edge list one round per edge position j (the j-th in-edge of every row), until no row has one left;
//   * the thread's sums are one row of per-chunk partials.
// k_f64_pg_fold adds the partial rows of PG_FOLD consecutive chunks in ascending order, k_f64_pg_final adds those group sums in
// ascending order into the gradient.  Chunk, group and round order are compile-time constants and the lists are the plan's canonical
// ones, so the summation order depends on the graph alone: the same call gives the same bits, on tiled and untiled plans alike.
// =============================================================================================
#define PG_ROWS 128   // rows per chunk = threads per workgroup
#define PG_RS 57      // doubles per LDS row: the widest round (update_neumann: 10 + 26 + 10 + 11); odd, so rows spread over the banks
#define PG_FOLD 64    // chunks per group of the first reduction stage
#define PG_MLP_RS 33  // psignn_mlp2_f64_backward: 16 + 16 + 1

// acc[j] += sum over the chunk's rows r (ascending) of buf[r][aoff + o] * buf[r][boff + k] for the entries e = tid + j * PG_ROWS
// < no * kw of one module, o = e / kw, k = e % kw; B's last column holds 1 (the bias).
template <int RS, int NA>
__device__ __forceinline__ void pg_acc(const double* buf, int aoff, int boff, int no, int kw, double* acc) {
#pragma unroll
  for (int j = 0; j < NA; ++j) {
    const int e = (int)threadIdx.x + j * PG_ROWS;
    if (e < no * kw) {
      const double *pa = buf + aoff + e / kw, *pb = buf + boff + e % kw;
      double s = acc[j];
#pragma unroll 8
      for (int r = 0; r < PG_ROWS; ++r) s = fma(pa[r * RS], pb[r * RS], s);
      acc[j] = s;
    }
  }
}
// the thread's entries into the chunk's partial row: weight (no, kw - 1) row-major at wofs, bias (no) at bofs
template <int NA>
__device__ __forceinline__ void pg_put(double* pt, int wofs, int bofs, int no, int kw, const double* acc) {
#pragma unroll
  for (int j = 0; j < NA; ++j) {
    const int e = (int)threadIdx.x + j * PG_ROWS;
    if (e < no * kw) {
      const int o = e / kw, k = e % kw;
      pt[k < kw - 1 ? wofs + o * (kw - 1) + k : bofs + o] = acc[j];
    }
  }
}

// One Phi module over one edge list of the chunk's rows: round j holds the j-th entry of every row's list.
// row: qm 0..9 | x_i 10..19, x_j 20..29, a 30..32, 1 | c 34..43 | relu(s) 44..53, 1
// TAN (the backward of the VJP): per edge position two sub-rounds, dA (x) B then A (x) dB, in the same row layout.
// c, dc: the lane's cotangents of the module's message sum and their tangents (read only when act).
template <bool TAN>
__device__ __forceinline__ void pg_edges(const double* __restrict__ Wp, bool act, const double* x, const double* dx, const double* cg,
                                         const double* dcg, const double* __restrict__ h, const double* __restrict__ t, int32_t beg,
                                         int32_t end, const int32_t* __restrict__ nbr, const double* __restrict__ attr, double* buf,
                                         double* row, double* pt, int base) {
  using L = W64<2>;
  double c[D], dc[D], q[D], dq[D], a1[2] = {0.0, 0.0}, a2[1] = {0.0};
#pragma unroll
  for (int k = 0; k < D; ++k) {
    c[k] = act ? cg[k] : 0.0;
    if (TAN) dc[k] = act ? dcg[k] : 0.0;
  }
  d64_w2t(Wp, c, q);
  if (TAN) d64_w2t(Wp, dc, dq);
  for (int32_t j = 0;; ++j) {
    const bool on = act && beg + j < end;
    if (!__syncthreads_or(on)) break;   // also the barrier behind the previous round's reads
    double xj[D], dxj[D], a[3], s[D], ds[D];
    if (on) {
      const int32_t i = beg + j;
      const int64_t u = nbr[i];
      d64_row(h, u, xj);
      if (TAN) d64_row(t, u, dxj);
#pragma unroll
      for (int k = 0; k < 3; ++k) a[k] = attr[3 * (int64_t)i + k];
      d64_pre(Wp, x, xj, a, s);
      if (TAN) d64_pre_tan(Wp, s, dx, dxj, ds);
      // (d) qm (x) [x_i, x_j, a, 1]; (d) c (x) [relu(s), 1]
#pragma unroll
      for (int k = 0; k < D; ++k) {
        row[k] = s[k] > 0.0 ? (TAN ? dq[k] : q[k]) : 0.0;
        row[10 + k] = x[k];
        row[20 + k] = xj[k];
        row[34 + k] = TAN ? dc[k] : c[k];
        row[44 + k] = fmax(s[k], 0.0);
      }
#pragma unroll
      for (int k = 0; k < 3; ++k) row[30 + k] = a[k];
      row[33] = 1.0;
      row[54] = 1.0;
    } else {
      for (int k = 0; k < 55; ++k) row[k] = 0.0;
    }
    __syncthreads();
    pg_acc<PG_RS, 2>(buf, 0, 10, D, L::EIN + 1, a1);
    pg_acc<PG_RS, 1>(buf, 34, 44, D, D + 1, a2);
    if (TAN) {
      __syncthreads();
      if (on) {   // qm (x) [dx_i, dx_j, 0, 0]; c (x) [1[s > 0] ds, 0]
#pragma unroll
        for (int k = 0; k < D; ++k) {
          row[k] = s[k] > 0.0 ? q[k] : 0.0;
          row[10 + k] = dx[k];
          row[20 + k] = dxj[k];
          row[34 + k] = c[k];
          row[44 + k] = ds[k];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) row[30 + k] = 0.0;
        row[54] = 0.0;
      }
      __syncthreads();
      pg_acc<PG_RS, 2>(buf, 0, 10, D, L::EIN + 1, a1);
      pg_acc<PG_RS, 1>(buf, 34, 44, D, D + 1, a2);
    }
  }
  pg_put<2>(pt, base + L::PHI_W1, base + L::PHI_B1, D, L::EIN + 1, a1);
  pg_put<1>(pt, base + L::PHI_W2, base + L::PHI_B2, D, D + 1, a2);
}

// One row of k_f64_pgrad, of one kind, as pass A of J^T w takes it: forward again, then back.  Leaves the factors of the rounds:
// cat, rp = relu(pre), gw = w and wy = w * yhat (LayerNorm's), gal, g, q and the cotangents c of the message sums.
template <int P, bool NEU>
__device__ __forceinline__ void pg_node_row(const double* W, int lofs, int nofs, int apply_ln, int64_t n, const double* x, double* gy,
                                            const double* h, const int32_t* csr_ptr, const int32_t* csr_nbr, const double* csr_attr,
                                            const int32_t* csc_ptr, const int32_t* csc_nbr, const double* csc_attr, const double* prb,
                                            const double* nrm, double* cat, double* rp, double* gw, double* wy, double& gal, double* g,
                                            double* q, double* c) {
  using L = W64<P>;
  double sv[D], y[D], al, dal;
  unsigned mask;
  d64_node_fwd<P, false, NEU>(W, lofs, nofs, n, x, nullptr, h, nullptr, csr_ptr, csr_nbr, csr_attr, csc_ptr, csc_nbr, csc_attr, prb, nrm,
                              cat, nullptr, al, dal, mask, rp, nullptr, sv, nullptr, y, nullptr);
  if (apply_ln) {   // laynorm.weight takes w * yhat, laynorm.bias w
    double yhat[D];
#pragma unroll
    for (int o = 0; o < D; ++o) gw[o] = gy[o];
    d64_ln_back(W + L::LN_G, y, gy, yhat);
#pragma unroll
    for (int o = 0; o < D; ++o) wy[o] = gw[o] * yhat[o];
  }
  d64_node_back_q<P, NEU>(W, lofs, nofs, mask, al, sv, gy, gal, g, q);
  d64_node_back_c<P, NEU>(W, lofs, nofs, gal, q, nullptr, c, nullptr);
}

// One layer's parameter gradient at (h, w), per chunk: part (chunks, W64<P>::total(1, MIXED)) in the layout of a single-layer block.
template <int P, bool MIXED>
__global__ __launch_bounds__(PG_ROWS) void k_f64_pgrad(int64_t N, const double* __restrict__ W, int lofs, int nofs, int apply_ln,
                                                       const int32_t* __restrict__ csr_ptr, const int32_t* __restrict__ csr_nbr,
                                                       const double* __restrict__ csr_attr, const int32_t* __restrict__ csc_ptr,
                                                       const int32_t* __restrict__ csc_nbr, const double* __restrict__ csc_attr,
                                                       const uint8_t* __restrict__ flags, const double* __restrict__ h,
                                                       const double* __restrict__ prb, const double* __restrict__ nrm,
                                                       const double* __restrict__ w, double* __restrict__ part) {
  using L = W64<P>;
  static_assert(10 + L::CAT + 1 + 1 <= PG_RS && 10 + L::NCAT + 1 + 10 + D + 1 <= PG_RS && D == 10, "LDS row of the rounds");
  __shared__ double buf[PG_ROWS * PG_RS];
  double* row = buf + threadIdx.x * PG_RS;
  double* pt = part + (int64_t)blockIdx.x * L::total(1, MIXED);
  const int64_t n = (int64_t)blockIdx.x * PG_ROWS + threadIdx.x;
  const uint8_t fl = n < N ? flags[n] : (uint8_t)FLAG_DIRICHLET;   // a row past the end gives what a Dirichlet row gives: nothing
  const bool live = !(fl & FLAG_DIRICHLET);
  const bool neu = MIXED && live && (fl & FLAG_NEUMANN);
  const bool upd = live && !neu;
  // the factors of the node rounds; a row is an update row or a Neumann row, so the two kinds share them:
  // q: cotangent of the hidden pre-activations; cat: the MLP's input; g: cotangent of the MLP's output; rp: relu(pre)
  double x[D], c[3 * D], q[D], cat[L::CAT], g[D], rp[D], wy[D], gw[D], gal = 0.0;
  int32_t rb = 0, re = 0, cb = 0, ce = 0;
#pragma unroll
  for (int k = 0; k < D; ++k) x[k] = q[k] = g[k] = rp[k] = wy[k] = gw[k] = 0.0;
#pragma unroll
  for (int k = 0; k < 3 * D; ++k) c[k] = 0.0;
#pragma unroll
  for (int k = 0; k < L::CAT; ++k) cat[k] = 0.0;
  if (live) {   // the node as pass A of J^T w takes it: forward again, then back; one kind of row per branch
    double gy[D];
    d64_row(h, n, x);
    d64_row(w, n, gy);
    rb = csr_ptr[n], re = csr_ptr[n + 1], cb = csc_ptr[n], ce = csc_ptr[n + 1];
    if (neu)
      pg_node_row<P, true>(W, lofs, nofs, apply_ln, n, x, gy, h, csr_ptr, csr_nbr, csr_attr, csc_ptr, csc_nbr, csc_attr, prb, nrm, cat, rp, gw,
                           wy, gal, g, q, c);
    else
      pg_node_row<P, false>(W, lofs, nofs, apply_ln, n, x, gy, h, csr_ptr, csr_nbr, csr_attr, csc_ptr, csc_nbr, csc_attr, prb, nrm, cat, rp,
                            gw, wy, gal, g, q, c);
  }
  const int ub = L::layer(0) + 2 * L::PHI_SZ;   // the update block of the partial row
  // ---- round 1, update rows: q 0..9 | cat 10 .. 10 + CAT, 1 | gal 44
  {
    double a1[3] = {0.0, 0.0, 0.0}, a2[1] = {0.0};
#pragma unroll
    for (int k = 0; k < D; ++k) row[k] = upd ? q[k] : 0.0;
#pragma unroll
    for (int k = 0; k < L::CAT; ++k) row[10 + k] = cat[k];
    row[10 + L::CAT] = 1.0;
    row[44] = upd ? gal : 0.0;
    __syncthreads();
    pg_acc<PG_RS, 3>(buf, 0, 10, D, L::CAT + 1, a1);
    pg_acc<PG_RS, 1>(buf, 44, 10, 1, L::CAT + 1, a2);
    pg_put<3>(pt, ub, ub + L::UPD_B1, D, L::CAT + 1, a1);
    pg_put<1>(pt, L::AL_W, L::AL_B, 1, L::CAT + 1, a2);
    __syncthreads();
  }
  // ---- round 2: g 0..9 | relu(pre) 10..19, 1 | w * yhat 21..30, w 31..40 (LayerNorm: every row that is not Dirichlet)
  {
    double a1[1] = {0.0}, s = 0.0;
#pragma unroll
    for (int k = 0; k < D; ++k) {
      row[k] = upd ? g[k] : 0.0;
      row[10 + k] = rp[k];
      row[21 + k] = wy[k];
      row[31 + k] = gw[k];
    }
    row[20] = 1.0;
    __syncthreads();
    pg_acc<PG_RS, 1>(buf, 0, 10, D, D + 1, a1);
    pg_put<1>(pt, ub + L::UPD_W2, ub + L::UPD_B2, D, D + 1, a1);
    if (threadIdx.x < 2 * D) {
      for (int r = 0; r < PG_ROWS; ++r) s += buf[r * PG_RS + 21 + threadIdx.x];
      pt[L::LN_G + threadIdx.x] = s;   // LN_G .. LN_B + D is one run
    }
    __syncthreads();
  }
  // ---- round 3, Neumann rows: q 0..9 | cat 10..34, 1 | g 36..45 | relu(pre) 46..55, 1
  if (MIXED) {
    const int nb = L::layer(1) + L::PHI_SZ;
    double a1[3] = {0.0, 0.0, 0.0}, a2[1] = {0.0};
#pragma unroll
    for (int k = 0; k < D; ++k) {
      row[k] = neu ? q[k] : 0.0;
      row[36 + k] = neu ? g[k] : 0.0;
      row[46 + k] = rp[k];
    }
#pragma unroll
    for (int k = 0; k < L::NCAT; ++k) row[10 + k] = cat[k];
    row[10 + L::NCAT] = 1.0;
    row[56] = 1.0;
    __syncthreads();
    pg_acc<PG_RS, 3>(buf, 0, 10, D, L::NCAT + 1, a1);
    pg_acc<PG_RS, 1>(buf, 36, 46, D, D + 1, a2);
    pg_put<3>(pt, nb, nb + L::NEU_B1, D, L::NCAT + 1, a1);
    pg_put<1>(pt, nb + L::NEU_W2, nb + L::NEU_B2, D, D + 1, a2);
  }
  // ---- the messages: Phi_to over the CSC list, Phi_from (Neumann rows: Phi_neumann) over the CSR list
  pg_edges<false>(W + lofs, upd, x, nullptr, c, nullptr, h, nullptr, cb, ce, csc_nbr, csc_attr, buf, row, pt, L::layer(0));
  pg_edges<false>(W + lofs + L::PHI_SZ, upd, x, nullptr, c + D, nullptr, h, nullptr, rb, re, csr_nbr, csr_attr, buf, row, pt,
                  L::layer(0) + L::PHI_SZ);
  if (MIXED) pg_edges<false>(W + nofs, neu, x, nullptr, c + 2 * D, nullptr, h, nullptr, rb, re, csr_nbr, csr_attr, buf, row, pt, L::layer(1));
}

// first stage: the partial rows of PG_FOLD consecutive chunks, added in ascending order into the first of them
__global__ __launch_bounds__(64) void k_f64_pg_fold(double* __restrict__ part, int64_t nch, int ps) {
  const int e = blockIdx.x * 64 + threadIdx.x;
  if (e >= ps) return;
  const int64_t c0 = (int64_t)blockIdx.y * PG_FOLD, c1 = c0 + PG_FOLD < nch ? c0 + PG_FOLD : nch;
  double s = part[c0 * ps + e];
#pragma unroll 8
  for (int64_t c = c0 + 1; c < c1; ++c) s += part[c * ps + e];
  part[c0 * ps + e] = s;
}
// second stage: the group sums in ascending order, added to the gradient.  Entry e of the single-layer layout goes to the shared
// section, to the layer's section at dl, or to the Neumann section at dn.
__global__ __launch_bounds__(64) void k_f64_pg_final(const double* __restrict__ part, int64_t nch, int ps, int shared, int layer,
                                                     int dl, int dn, double* __restrict__ grad) {
  const int e = blockIdx.x * 64 + threadIdx.x;
  if (e >= ps) return;
  double s = part[e];
#pragma unroll 8
  for (int64_t c = PG_FOLD; c < nch; c += PG_FOLD) s += part[c * ps + e];
  const int d = e < shared ? e : e < shared + layer ? dl + (e - shared) : dn + (e - shared - layer);
  grad[d] += s;
}

// w^T df/dh_initial of one layer: the Dirichlet rows of the cotangent on the layer's output, 0 elsewhere
__global__ __launch_bounds__(256) void k_f64_pg_init(int64_t N, const uint8_t* __restrict__ flags, const double* __restrict__ w,
                                                     int accumulate, double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N * D) return;
  if (flags[i / D] & FLAG_DIRICHLET)
    out[i] = accumulate ? out[i] + w[i] : w[i];
  else if (!accumulate)
    out[i] = 0.0;
}

extern "C" int psignn_f64_param_vjp_chunk_rows(void) { return PG_ROWS; }

static inline int64_t pg_part_doubles(const psignn_f64* f) {
  return cdiv(f->p->N, PG_ROWS) * (f->p->mixed ? W64<3>::total(1, true) : W64<2>::total(1, false));
}

extern "C" int64_t psignn_f64_param_vjp_workspace_doubles(const psignn_f64_t* f, int n_layers) {
  if (!f || n_layers < 1) return -1;
  return psignn_f64_deriv_workspace_doubles(f, n_layers, 1) + pg_part_doubles(f);   // J^T w's own, then the per-chunk partials
}

static void pg_reduce(double* part, int64_t nch, int ps, int shared, int layer, int dl, int dn, double* grad, hipStream_t st) {
  PROF_BYTES(nch * ps * 8);
  LAUNCH("k_f64_pg_fold", st,
         (k_f64_pg_fold<<<dim3((unsigned)cdiv(ps, 64), (unsigned)cdiv(nch, PG_FOLD)), 64, 0, st>>>(part, nch, ps)));
  PROF_BYTES(cdiv(nch, PG_FOLD) * ps * 8 + 16 * ps);
  LAUNCH("k_f64_pg_final", st,
         (k_f64_pg_final<<<(unsigned)cdiv(ps, 64), 64, 0, st>>>(part, nch, ps, shared, layer, dl, dn, grad)));
}

// layer l's gradient at (h, w) added to grad, and (init) its share of w^T df/dh_initial
static void pgrad_launch(const psignn_f64* f, const double* W, int nl, int l, int apply_ln, const double* h, const double* prb,
                         const double* nrm, const double* w, double* part, double* grad, double* init, int init_acc, hipStream_t st) {
  const psignn_plan* p = f->p;
  const int64_t nch = cdiv(p->N, PG_ROWS);
  // both edge lists twice (the node's forward, then the rounds: neighbour id, 3 attributes, the neighbour's row), per node h, w,
  // flag, pointers and problem data; the partial rows
  PROF_BYTES(4 * p->Ep * (4 + 24 + 8 * D) + p->N * (16 * D + 8 * (p->mixed ? 5 : 2) + 17) + pg_part_doubles(f) * 8);
  F64_FAMILY(p->mixed, LAUNCH("k_f64_pgrad", st,
                              (k_f64_pgrad<P, MIXED><<<(unsigned)nch, PG_ROWS, 0, st>>>(p->N, W, L::layer(l), L::layer(nl), apply_ln,
                                                                                       F64_EDGES(f), h, prb, nrm, w, part)));
             pg_reduce(part, nch, L::total(1, MIXED), L::SHARED, L::LAYER, L::layer(l), L::layer(nl), grad, st));
  if (init) {
    PROF_BYTES(p->N * (1 + 16 * D));
    LAUNCH("k_f64_pg_init", st,
           (k_f64_pg_init<<<(unsigned)cdiv(p->N * D, 256), 256, 0, st>>>(p->N, p->flags, w, init_acc, init)));
  }
}

extern "C" int psignn_f64_param_vjp(psignn_f64_t* f, const double* W, int nl, const double* h, const double* h0, const double* prb,
                                    const double* nrm, const double* w, double* d_grad, double* d_out_h, double* d_out_init,
                                    double* work, int64_t work_doubles, void* stream) {
  ARG_CHECK(f && W && h && h0 && prb && w && d_grad && d_out_h, "NULL argument");
  ARG_CHECK(nl >= 1 && nl <= 64, "n_layers out of range");
  ARG_CHECK(!f->p->mixed || nrm, "mixed plan needs unit normals");
  ARG_CHECK(d_out_h != h && d_out_h != w, "d_out_h must not alias h or w");
  ARG_CHECK(d_out_init != h && d_out_init != w && d_out_init != d_out_h, "d_out_init must not alias h, w or d_out_h");
  const int rc = work_check(__func__, psignn_f64_param_vjp_workspace_doubles(f, nl), work, work_doubles);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipMemsetAsync(d_grad, 0, sizeof(double) * psignn_f64_weights_size(f->p->mixed, nl), st));
  if (f->p->N == 0) return PSIGNN_OK;
  const int64_t row = f->p->N * D;
  double *loc = work, *C = work + row, *part = work + psignn_f64_deriv_workspace_doubles(f, nl, 1);
  const bool chain = f64_chain(f, nl);   // states, pp: as psignn_f64_vjp lays them out
  double *states = chain ? work + 3 * row : nullptr, *pp = chain ? work + (3 + nl - 1) * row : nullptr;
  // layer l's gradient at (h_l, w_{l+1}) before w_l = J_l^T w_{l+1}.  mixed: only the last layer's iteration reaches the output, the
  // earlier layers' sections stay zero
  f64_walk_back(f, W, nl, h, nullptr, h0, prb, states, nullptr, w, pp, d_out_h, nullptr, st,
                [&](int l, bool, const double* hl, const double*, const double* wl, double* dst) {
                  pgrad_launch(f, W, nl, l, l == nl - 1, hl, prb, nrm, wl, part, d_grad, d_out_init, l != nl - 1, st);
                  vjp_launch(f, W, nl, l, l == nl - 1, hl, prb, nrm, wl, loc, C, nullptr, dst, nullptr, st);
                });
  HIP_TRY(hipGetLastError());
  return PSIGNN_OK;
}

// ---------------------------------------------------------------------------------------------
// backward of psignn_mlp2_f64: y = W2 relu(W1 x + b1) + b2.  One row per lane, chunks of PG_ROWS rows, the same two-stage sum.
// round 1: gh 0..15 | x 16 .. 16 + din, 1        round 2: gy 0..15 | relu(pre) 16 .. 16 + hid, 1
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PG_ROWS) void k_mlp2_f64_backward(const double* __restrict__ x, const double* __restrict__ gy, int64_t n,
                                                               int din, int hid, int dout, const double* __restrict__ w1,
                                                               const double* __restrict__ b1, const double* __restrict__ w2,
                                                               double* __restrict__ gx, double* __restrict__ part) {
  __shared__ double buf[PG_ROWS * PG_MLP_RS];
  double* row = buf + threadIdx.x * PG_MLP_RS;
  const int ps = hid * din + hid + dout * hid + dout;
  double* pt = part + (int64_t)blockIdx.x * ps;
  const int64_t i = (int64_t)blockIdx.x * PG_ROWS + threadIdx.x;
  const bool live = i < n;
  double xi[16], go[16], gh[16], rp[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    xi[k] = live && k < din ? x[i * din + k] : 0.0;
    go[k] = live && k < dout ? gy[i * dout + k] : 0.0;
  }
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    double s = 0.0, t = 0.0;
    if (j < hid) {
      s = b1[j];
#pragma unroll
      for (int k = 0; k < 16; ++k)
        if (k < din) s = fma(w1[j * din + k], xi[k], s);
#pragma unroll
      for (int o = 0; o < 16; ++o)
        if (o < dout) t = fma(w2[o * hid + j], go[o], t);
    }
    rp[j] = live ? fmax(s, 0.0) : 0.0;
    gh[j] = live && s > 0.0 ? t : 0.0;
  }
  if (gx && live) {
    for (int k = 0; k < din; ++k) {
      double s = 0.0;
#pragma unroll
      for (int j = 0; j < 16; ++j)
        if (j < hid) s = fma(w1[j * din + k], gh[j], s);
      gx[i * din + k] = s;
    }
  }
  double a1[3] = {0.0, 0.0, 0.0}, a2[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    row[k] = gh[k];
    row[16 + k] = xi[k];
  }
  row[16 + din] = 1.0;
  __syncthreads();
  pg_acc<PG_MLP_RS, 3>(buf, 0, 16, hid, din + 1, a1);
  pg_put<3>(pt, 0, hid * din, hid, din + 1, a1);
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    row[k] = go[k];
    row[16 + k] = rp[k];
  }
  row[16 + hid] = 1.0;
  __syncthreads();
  pg_acc<PG_MLP_RS, 3>(buf, 0, 16, dout, hid + 1, a2);
  pg_put<3>(pt, hid * din + hid, hid * din + hid + dout * hid, dout, hid + 1, a2);
}

extern "C" int64_t psignn_mlp2_f64_backward_workspace_doubles(int64_t n, int din, int hid, int dout) {
  if (n < 0 || din < 1 || din > 16 || hid < 1 || hid > 16 || dout < 1 || dout > 16) return -1;
  return cdiv(n, PG_ROWS) * (hid * din + hid + dout * hid + dout);
}

extern "C" int psignn_mlp2_f64_backward(const double* x, const double* gy, int64_t n, int din, int hid, int dout, const double* w1,
                                        const double* b1, const double* w2, double* gx, double* gflat, double* work,
                                        int64_t work_doubles, void* stream) {
  ARG_CHECK(x && gy && w1 && b1 && w2 && gflat, "NULL argument");
  ARG_CHECK(n >= 0 && din >= 1 && din <= 16 && hid >= 1 && hid <= 16 && dout >= 1 && dout <= 16, "bad sizes");
  ARG_CHECK(gx != x && gx != gy, "gx must not alias x or gy");
  const int rc = work_check(__func__, psignn_mlp2_f64_backward_workspace_doubles(n, din, hid, dout), work, work_doubles);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int ps = hid * din + hid + dout * hid + dout;
  HIP_TRY(hipMemsetAsync(gflat, 0, sizeof(double) * ps, st));
  if (n == 0) return PSIGNN_OK;
  const int64_t nch = cdiv(n, PG_ROWS);
  PROF_BYTES(n * 8 * (2 * din + dout) + nch * ps * 8);
  LAUNCH("k_mlp2_f64_backward", st,
         (k_mlp2_f64_backward<<<(unsigned)nch, PG_ROWS, 0, st>>>(x, gy, n, din, hid, dout, w1, b1, w2, gx, work)));
  pg_reduce(work, nch, ps, ps, 0, 0, 0, gflat, st);
  HIP_TRY(hipGetLastError());
  return PSIGNN_OK;
}

// =============================================================================================
// Backward of the VJP in float64: for a probe v and a constant gbar, psi(theta, h) = <gbar, J_f(h)^T v>; wanted are its gradient with
// respect to every deqdss.f.* tensor and to h, and J^T v itself.
//
// replaces: the double backward loss.backward() runs for the Jacobian regulariser, in double precision -- jac_loss_estimate
//           (dirichlet/psignn/model.py:416-435: autograd.grad(f0, z0, v, create_graph=True), then the backward of |v^T J|^2 / numel);
//           mixed/psignn/model.py likewise.
//
// psi is the directional derivative along gbar of phi(theta, h) = <v, f(h)>, so its gradient is the tangent along dh = gbar of the
// reverse pass above: every cotangent of pass A and of k_f64_pgrad travels with its tangent.  ReLU masks are constants of the tangent
// (ReLU has no curvature), so what is left is the curvature of the gate (sigmoid x update) and of LayerNorm.
//   k_f64_jr, per receiving node n in chunks of PG_ROWS rows: the node's forward with its tangent (d64_phi<true>), w_n and dw_n back
//     through LayerNorm, gate and update (or update_neumann) with the product rule at every step; dloc[n], the tangent of the node-
//     local part of J^T w; C[n] and dC[n], the cotangents of the message sums and their tangents; and the rounds of k_f64_pgrad, each
//     run twice, dA (x) B then A (x) dB, into the same per-chunk partial row.
//   pass B is linear in (loc, C) at fixed masks: k_f64_vjp_edge on (dloc, dC) is the tangent of J^T w.
//   k_f64_pg_fold / k_f64_pg_final add the partial rows as they do for the first-order gradient.
// A multi-layer dirichlet block is a chain: forward with k_f64_jvp_layer for (h_k, t_k), t_0 = gbar, then backwards with
// (w_{k+1}, dw_{k+1}) -> (w_k, dw_k), w_L = v, dw_L = 0.  No atomics, a summation order that depends on the graph alone.
// =============================================================================================
// One layer at (h, t, w, dw): dloc (N, D), C and dC (N, CW) and the chunk's partial row of the parameter part.  dw NULL: zero.
// The node's forward and reverse with a tangent stand here in this kernel's own words.  With d64_node_fwd<P, true, .> of f64_node.h
// and tangent forms of its reverse pieces in their place, all three instantiations compiled without scratch and without spills, and
// still the sums of laynorm.* came back wrong and different from call to call on the device; the cause was not found.
// ROWS: 0 every row (dirichlet plans); a mixed plan takes two passes, 1 the update rows (and zeros for every other row of dloc, C,
// dC), then 2 the Neumann rows, each with a partial row of its own sections and zeros elsewhere.  One kind of row per pass keeps
// the node's block on one code path and inside the register file: a value spilled inside a divergent region and read after it is
// not safe for the lanes that sat the region out.
template <int P, bool MIXED, int ROWS>
__global__ __launch_bounds__(PG_ROWS) void k_f64_jr(int64_t N, const double* __restrict__ W, int lofs, int nofs, int apply_ln,
                                                    const int32_t* __restrict__ csr_ptr, const int32_t* __restrict__ csr_nbr,
                                                    const double* __restrict__ csr_attr, const int32_t* __restrict__ csc_ptr,
                                                    const int32_t* __restrict__ csc_nbr, const double* __restrict__ csc_attr,
                                                    const uint8_t* __restrict__ flags, const double* __restrict__ h,
                                                    const double* __restrict__ t, const double* __restrict__ prb,
                                                    const double* __restrict__ nrm, const double* __restrict__ w,
                                                    const double* __restrict__ dw, double* __restrict__ C, double* __restrict__ dloc,
                                                    double* __restrict__ dC, double* __restrict__ part) {
  using L = W64<P>;
  constexpr int CW = MIXED ? 3 * D : 2 * D;
  static_assert(10 + L::CAT + 1 + 1 <= PG_RS && 10 + L::NCAT + 1 + 10 + D + 1 <= PG_RS && D == 10, "LDS row of the rounds");
  __shared__ double buf[PG_ROWS * PG_RS];
  double* row = buf + threadIdx.x * PG_RS;
  double* pt = part + (int64_t)blockIdx.x * L::total(1, MIXED);
  const int64_t n = (int64_t)blockIdx.x * PG_ROWS + threadIdx.x;
  const uint8_t fl = n < N ? flags[n] : (uint8_t)FLAG_DIRICHLET;   // a row past the end gives what a Dirichlet row gives: nothing
  static_assert(MIXED ? ROWS == 1 || ROWS == 2 : ROWS == 0, "a mixed plan takes the two passes, a dirichlet plan the one");
  const bool neu_row = MIXED && (fl & FLAG_NEUMANN);
  const bool live = !(fl & FLAG_DIRICHLET) && (ROWS == 0 || neu_row == (ROWS == 2));   // the rows of this pass
  const bool neu = ROWS == 2 && live;
  const bool upd = ROWS != 2 && live;
  // the factors of the node rounds and their tangents (names as in k_f64_pgrad); lnA: d (w * yhat), lnB: dw.  Every round selects
  // on live / upd / neu where it writes them: what a lane that skipped the block below holds in these registers is never read.
  double x[D], dx[D], q[D], dq[D], cat[L::CAT], dcat[3 * D], g[D], dg[D], rp[D], drp[D], lnA[D], lnB[D], dgy[D], gal = 0.0, dgal = 0.0;
  int32_t rb = 0, re = 0, cb = 0, ce = 0;
#pragma unroll
  for (int k = 0; k < D; ++k) x[k] = dx[k] = q[k] = dq[k] = g[k] = dg[k] = rp[k] = drp[k] = lnA[k] = lnB[k] = dgy[k] = 0.0;
#pragma unroll
  for (int k = 0; k < L::CAT; ++k) cat[k] = 0.0;
#pragma unroll
  for (int k = 0; k < 3 * D; ++k) dcat[k] = 0.0;
  if (live) {
    double gy[D], y[D], dy[D], sv[D], dsv[D];
    unsigned mask = 0;
    d64_row(h, n, x);
    d64_row(t, n, dx);
    d64_row(w, n, gy);
#pragma unroll
    for (int k = 0; k < D; ++k) dgy[k] = dw ? dw[n * D + k] : 0.0;
    rb = csr_ptr[n], re = csr_ptr[n + 1], cb = csc_ptr[n], ce = csc_ptr[n + 1];
    double al = 1.0, dal = 0.0;
    const double* Wm = neu ? W + nofs + L::PHI_SZ : W + lofs + 2 * L::PHI_SZ;   // W1 | b1 | W2 | b2 of the row's MLP
    int ncat, ob1, ow2, ob2;
#pragma unroll
    for (int k = 0; k < D; ++k) {
      cat[k] = x[k];
      dcat[k] = dx[k];
    }
    if (neu) {
      d64_phi<true>(W + nofs, x, dx, h, t, rb, re, csr_nbr, csr_attr, cat + D, dcat + D);
#pragma unroll
      for (int k = 0; k < P; ++k) cat[2 * D + k] = prb[n * P + k];
      cat[2 * D + P] = nrm[2 * n];
      cat[2 * D + P + 1] = nrm[2 * n + 1];
      ncat = L::NCAT, ob1 = L::NEU_B1, ow2 = L::NEU_W2, ob2 = L::NEU_B2;
    } else {
      d64_phi<true>(W + lofs, x, dx, h, t, cb, ce, csc_nbr, csc_attr, cat + D, dcat + D);
      d64_phi<true>(W + lofs + L::PHI_SZ, x, dx, h, t, rb, re, csr_nbr, csr_attr, cat + 2 * D, dcat + 2 * D);
#pragma unroll
      for (int k = 0; k < P; ++k) cat[3 * D + k] = prb[n * P + k];
      al = W[L::AL_B];
#pragma unroll
      for (int k = 0; k < L::CAT; ++k) al = fma(W[L::AL_W + k], cat[k], al);
      al = d64_sigmoid(al);
#pragma unroll
      for (int k = 0; k < 3 * D; ++k) dal = fma(W[L::AL_W + k], dcat[k], dal);
      dal *= al * (1.0 - al);
      ncat = L::CAT, ob1 = L::UPD_B1, ow2 = L::UPD_W2, ob2 = L::UPD_B2;
    }
    const int nd = neu ? 2 * D : 3 * D;   // inputs of the MLP that carry a tangent
#pragma unroll
    for (int o = 0; o < D; ++o) {
      double s = Wm[ob1 + o], r = 0.0;
#pragma unroll
      for (int k = 0; k < L::CAT; ++k)
        if (k < ncat) s = fma(Wm[o * ncat + k], cat[k], s);
#pragma unroll
      for (int k = 0; k < 3 * D; ++k)
        if (k < nd) r = fma(Wm[o * ncat + k], dcat[k], r);
      if (s > 0.0) mask |= 1u << o;
      rp[o] = fmax(s, 0.0);
      drp[o] = s > 0.0 ? r : 0.0;
    }
#pragma unroll
    for (int o = 0; o < D; ++o) {
      double s = Wm[ob2 + o], r = 0.0;
#pragma unroll
      for (int k = 0; k < D; ++k) {
        s = fma(Wm[ow2 + o * D + k], rp[k], s);
        r = fma(Wm[ow2 + o * D + k], drp[k], r);
      }
      sv[o] = s;
      dsv[o] = r;
      y[o] = neu ? s : x[o] + al * s;
      dy[o] = neu ? r : dx[o] + dal * s + al * r;
    }
    if (apply_ln) {
      double yhat[D], dyh[D];
#pragma unroll
      for (int o = 0; o < D; ++o) {
        lnA[o] = gy[o];
        lnB[o] = dgy[o];
      }
      d64_ln_back_tan(W + L::LN_G, y, dy, gy, dgy, yhat, dyh);
#pragma unroll
      for (int o = 0; o < D; ++o) lnA[o] = fma(lnB[o], yhat[o], lnA[o] * dyh[o]);
    }
    if (!neu) {   // y = x + al * s: the gate's pre-activation gets (gy . s) al (1 - al)
      double dot = 0.0, ddot = 0.0;
#pragma unroll
      for (int o = 0; o < D; ++o) {
        dot = fma(gy[o], sv[o], dot);
        ddot = fma(dgy[o], sv[o], fma(gy[o], dsv[o], ddot));
      }
      const double sp = al * (1.0 - al);
      gal = dot * sp;
      dgal = fma(ddot, sp, dot * (1.0 - 2.0 * al) * dal);
    }
#pragma unroll
    for (int o = 0; o < D; ++o) {
      g[o] = al * gy[o];
      dg[o] = fma(dal, gy[o], al * dgy[o]);
    }
#pragma unroll
    for (int k = 0; k < D; ++k) {
      double s = 0.0, r = 0.0;
#pragma unroll
      for (int o = 0; o < D; ++o) {
        s = fma(Wm[ow2 + o * D + k], g[o], s);
        r = fma(Wm[ow2 + o * D + k], dg[o], r);
      }
      const bool pos = (mask >> k) & 1u;
      q[k] = pos ? s : 0.0;
      dq[k] = pos ? r : 0.0;
    }
  }
  const int ub = L::layer(0) + 2 * L::PHI_SZ;   // the update block of the partial row
  // the rounds, in the order that lets go of the most registers first: 2 (LayerNorm), 3 (Neumann), 1 (update W1 and gate)
  // ---- round 2: g 0..9 | relu(pre) 10..19, 1 | d (w * yhat) 21..30, dw 31..40 (LayerNorm: every row that is not Dirichlet)
  {
    double a1[1] = {0.0}, s = 0.0;
#pragma unroll
    for (int k = 0; k < D; ++k) {
      row[k] = upd ? dg[k] : 0.0;
      row[10 + k] = live ? rp[k] : 0.0;
      row[21 + k] = live ? lnA[k] : 0.0;
      row[31 + k] = live ? lnB[k] : 0.0;
    }
    row[20] = 1.0;
    __syncthreads();
    pg_acc<PG_RS, 1>(buf, 0, 10, D, D + 1, a1);
    if (threadIdx.x < 2 * D) {
      for (int r = 0; r < PG_ROWS; ++r) s += buf[r * PG_RS + 21 + threadIdx.x];
      pt[L::LN_G + threadIdx.x] = s;   // LN_G .. LN_B + D is one run
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < D; ++k) {
      row[k] = upd ? g[k] : 0.0;
      row[10 + k] = live ? drp[k] : 0.0;
    }
    row[20] = 0.0;
    __syncthreads();
    pg_acc<PG_RS, 1>(buf, 0, 10, D, D + 1, a1);
    pg_put<1>(pt, ub + L::UPD_W2, ub + L::UPD_B2, D, D + 1, a1);
    __syncthreads();
  }
  // ---- round 3, Neumann rows: q 0..9 | cat 10..34, 1 | g 36..45 | relu(pre) 46..55, 1
  if (MIXED) {
    const int nb = L::layer(1) + L::PHI_SZ;
    double a1[3] = {0.0, 0.0, 0.0}, a2[1] = {0.0};
    if (ROWS == 2) {   // the update pass leaves zeros in these sections
#pragma unroll
      for (int k = 0; k < D; ++k) {
        row[k] = neu ? dq[k] : 0.0;
        row[36 + k] = neu ? dg[k] : 0.0;
        row[46 + k] = live ? rp[k] : 0.0;
      }
#pragma unroll
      for (int k = 0; k < L::NCAT; ++k) row[10 + k] = live ? cat[k] : 0.0;
      row[10 + L::NCAT] = 1.0;
      row[56] = 1.0;
      __syncthreads();
      pg_acc<PG_RS, 3>(buf, 0, 10, D, L::NCAT + 1, a1);
      pg_acc<PG_RS, 1>(buf, 36, 46, D, D + 1, a2);
      __syncthreads();
#pragma unroll
      for (int k = 0; k < D; ++k) {
        row[k] = neu ? q[k] : 0.0;
        row[36 + k] = neu ? g[k] : 0.0;
        row[46 + k] = live ? drp[k] : 0.0;
      }
#pragma unroll
      for (int k = 0; k < L::NCAT + 1; ++k) row[10 + k] = live && k < 2 * D ? dcat[k] : 0.0;
      row[56] = 0.0;
      __syncthreads();
      pg_acc<PG_RS, 3>(buf, 0, 10, D, L::NCAT + 1, a1);
      pg_acc<PG_RS, 1>(buf, 36, 46, D, D + 1, a2);
    }
    pg_put<3>(pt, nb, nb + L::NEU_B1, D, L::NCAT + 1, a1);
    pg_put<1>(pt, nb + L::NEU_W2, nb + L::NEU_B2, D, D + 1, a2);
    __syncthreads();
  }
  // ---- round 1, update rows: q 0..9 | cat 10 .. 10 + CAT, 1 | gal 44; first (dq, dgal) with cat, then (q, gal) with dcat
  {
    double a1[3] = {0.0, 0.0, 0.0}, a2[1] = {0.0};
    if (ROWS != 2) {   // the Neumann pass leaves zeros in these sections
#pragma unroll
      for (int k = 0; k < D; ++k) row[k] = upd ? dq[k] : 0.0;
#pragma unroll
      for (int k = 0; k < L::CAT; ++k) row[10 + k] = live ? cat[k] : 0.0;
      row[10 + L::CAT] = 1.0;
      row[44] = upd ? dgal : 0.0;
      __syncthreads();
      pg_acc<PG_RS, 3>(buf, 0, 10, D, L::CAT + 1, a1);
      pg_acc<PG_RS, 1>(buf, 44, 10, 1, L::CAT + 1, a2);
      __syncthreads();
#pragma unroll
      for (int k = 0; k < D; ++k) row[k] = upd ? q[k] : 0.0;
#pragma unroll
      for (int k = 0; k < 3 * D; ++k) row[10 + k] = live ? dcat[k] : 0.0;
#pragma unroll
      for (int k = 3 * D; k < L::CAT + 1; ++k) row[10 + k] = 0.0;
      row[44] = upd ? gal : 0.0;
      __syncthreads();
      pg_acc<PG_RS, 3>(buf, 0, 10, D, L::CAT + 1, a1);
      pg_acc<PG_RS, 1>(buf, 44, 10, 1, L::CAT + 1, a2);
    }
    pg_put<3>(pt, ub, ub + L::UPD_B1, D, L::CAT + 1, a1);
    pg_put<1>(pt, L::AL_W, L::AL_B, 1, L::CAT + 1, a2);
    __syncthreads();
  }
  // ---- the cotangents of the message sums and of x with their tangents, after the node rounds have let go of their factors
  if (live) {
    double c[CW], dc[CW], dgx[D], qq[D];
#pragma unroll
    for (int k = 0; k < CW; ++k) c[k] = dc[k] = 0.0;
    const double* Wm = neu ? W + nofs + L::PHI_SZ : W + lofs + 2 * L::PHI_SZ;
    if (neu) {
#pragma unroll
      for (int k = 0; k < D; ++k) {
        double s = 0.0, r = 0.0, u = 0.0;
#pragma unroll
        for (int o = 0; o < D; ++o) {
          s = fma(Wm[o * L::NCAT + D + k], q[o], s);
          r = fma(Wm[o * L::NCAT + D + k], dq[o], r);
          u = fma(Wm[o * L::NCAT + k], dq[o], u);
        }
        c[CW - D + k] = s;
        dc[CW - D + k] = r;
        dgx[k] = u;
      }
      d64_w2t(W + nofs, dc + CW - D, qq);
      d64_phi_vjp_xi(W + nofs, x, h, rb, re, csr_nbr, csr_attr, qq, dgx);
    } else {
#pragma unroll
      for (int k = 0; k < 3 * D; ++k) {
        double s = W[L::AL_W + k] * gal, r = W[L::AL_W + k] * dgal;
#pragma unroll
        for (int o = 0; o < D; ++o) {
          s = fma(Wm[o * L::CAT + k], q[o], s);
          r = fma(Wm[o * L::CAT + k], dq[o], r);
        }
        if (k < D) {
          dgx[k] = dgy[k] + r;
        } else {
          c[k - D] = s;
          dc[k - D] = r;
        }
      }
      d64_w2t(W + lofs, dc, qq);
      d64_phi_vjp_xi(W + lofs, x, h, cb, ce, csc_nbr, csc_attr, qq, dgx);
      d64_w2t(W + lofs + L::PHI_SZ, dc + D, qq);
      d64_phi_vjp_xi(W + lofs + L::PHI_SZ, x, h, rb, re, csr_nbr, csr_attr, qq, dgx);
    }
#pragma unroll
    for (int k = 0; k < D; ++k) dloc[n * D + k] = dgx[k];
#pragma unroll
    for (int k = 0; k < CW; ++k) {
      C[n * CW + k] = c[k];
      dC[n * CW + k] = dc[k];
    }
  } else if (ROWS != 2 && n < N) {   // pass 2 leaves the rows of pass 1 alone
#pragma unroll
    for (int k = 0; k < D; ++k) dloc[n * D + k] = 0.0;
#pragma unroll
    for (int k = 0; k < CW; ++k) C[n * CW + k] = dC[n * CW + k] = 0.0;
  }
  // ---- the messages: Phi_to over the CSC list, Phi_from (Neumann rows: Phi_neumann) over the CSR list; c and dc from the rows above
  const double *cg = C + (live ? n : 0) * CW, *dcg = dC + (live ? n : 0) * CW;
  pg_edges<true>(W + lofs, upd, x, dx, cg, dcg, h, t, cb, ce, csc_nbr, csc_attr, buf, row, pt, L::layer(0));
  pg_edges<true>(W + lofs + L::PHI_SZ, upd, x, dx, cg + D, dcg + D, h, t, rb, re, csr_nbr, csr_attr, buf, row, pt, L::layer(0) + L::PHI_SZ);
  if (MIXED) pg_edges<true>(W + nofs, neu, x, dx, cg + 2 * D, dcg + 2 * D, h, t, rb, re, csr_nbr, csr_attr, buf, row, pt, L::layer(1));
}

extern "C" int64_t psignn_f64_vjp_backward_workspace_doubles(const psignn_f64_t* f, int n_layers) {
  if (!f || n_layers < 1) return -1;
  const int64_t row = f->p->N * D;
  const int cw = f->p->mixed ? 3 : 2;
  // loc, C of J^T v; dloc, dC; a chain: the states and their tangents, the ping-pongs of w and dw; the per-chunk partials
  return row * (2 + 2 * cw) + (f64_chain(f, n_layers) ? row * (2 * (n_layers - 1) + 4) : 0) + pg_part_doubles(f);
}

// layer l at (h, t, w, dw): its share of the parameter part added to grad, and out = the tangent of J_l(h)^T w
static void jr_launch(const psignn_f64* f, const double* W, int nl, int l, int apply_ln, const double* h, const double* t,
                      const double* prb, const double* nrm, const double* w, const double* dw, double* C, double* dloc, double* dC,
                      double* part, double* grad, double* out, hipStream_t st) {
  const psignn_plan* p = f->p;
  const int64_t nch = cdiv(p->N, PG_ROWS);
  const int cw = p->mixed ? 3 * D : 2 * D;
  // both edge lists three times (the forward with its tangent, the x_i side, the rounds: neighbour id, 3 attributes, the neighbour's
  // row and -- twice -- its tangent row), per node h, t, w, dw, dloc, C and dC written and read again, flag, pointers and problem
  // data; the partial rows
  PROF_BYTES(2 * p->Ep * (3 * (4 + 24) + 40 * D) + p->N * (8 * (5 * D + 4 * cw) + 8 * (p->mixed ? 5 : 2) + 17) + pg_part_doubles(f) * 8);
  F64_FAMILY(p->mixed, LAUNCH("k_f64_jr", st,
                              (k_f64_jr<P, MIXED, MIXED ? 1 : 0><<<(unsigned)nch, PG_ROWS, 0, st>>>(
                                  p->N, W, L::layer(l), L::layer(nl), apply_ln, F64_EDGES(f), h, t, prb, nrm, w, dw, C, dloc, dC, part)));
             pg_reduce(part, nch, L::total(1, MIXED), L::SHARED, L::LAYER, L::layer(l), L::layer(nl), grad, st));
  if (p->mixed) {
    // the Neumann rows: per node flag and pointers, the partial rows once more; the edge reads of the few Neumann rows are not
    // counted (the host does not know how many there are)
    using L = W64<3>;
    PROF_BYTES(p->N * 17 + pg_part_doubles(f) * 8);
    LAUNCH("k_f64_jr_neumann", st,
           (k_f64_jr<3, true, 2><<<(unsigned)nch, PG_ROWS, 0, st>>>(p->N, W, L::layer(l), L::layer(nl), apply_ln, F64_EDGES(f), h, t,
                                                                    prb, nrm, w, dw, C, dloc, dC, part)));
    pg_reduce(part, nch, L::total(1, true), L::SHARED, L::LAYER, L::layer(l), L::layer(nl), grad, st);
  }
  vjp_edge_launch(f, W, nl, l, h, dloc, dC, nullptr, out, nullptr, st);   // pass B on (dloc, dC), masks at h
}

// d_dinit (may be NULL) = d psi / d h_initial: the Dirichlet rows of the tangents of the cotangents on the states h_1 .. h_{L-1} of a
// multi-layer dirichlet block (those rows are copies of h_initial, and J_f is evaluated at them); zeros for every other block, whose
// Jacobian does not depend on h_initial.
static int vjp_backward_impl(const char* who, psignn_f64_t* f, const double* W, int nl, const double* h, const double* h0,
                             const double* prb, const double* nrm, const double* v, const double* gbar, double* d_grad, double* d_dh,
                             double* d_jtv, double* d_dinit, double* work, int64_t work_doubles, void* stream) {
  ARG_CHECK_AS(who, f && W && h && h0 && prb && v && gbar && d_grad && d_dh, "NULL argument");
  ARG_CHECK_AS(who, nl >= 1 && nl <= 64, "n_layers out of range");
  ARG_CHECK_AS(who, !f->p->mixed || nrm, "mixed plan needs unit normals");
  ARG_CHECK_AS(who, d_dh != h && d_dh != v && d_dh != gbar, "d_dh must not alias h, v or gbar");
  ARG_CHECK_AS(who, d_jtv != h && d_jtv != v && d_jtv != gbar && d_jtv != d_dh, "d_jtv must not alias h, v, gbar or d_dh");
  ARG_CHECK_AS(who, !d_dinit || (d_dinit != h && d_dinit != v && d_dinit != gbar && d_dinit != d_dh && d_dinit != d_jtv),
            "d_dinit must not alias h, v, gbar, d_dh or d_jtv");
  const int rc = work_check(who, psignn_f64_vjp_backward_workspace_doubles(f, nl), work, work_doubles);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipMemsetAsync(d_grad, 0, sizeof(double) * psignn_f64_weights_size(f->p->mixed, nl), st));
  if (f->p->N == 0) return PSIGNN_OK;
  const int64_t row = f->p->N * D;
  const int cw = f->p->mixed ? 3 : 2;
  const bool chain = f64_chain(f, nl);
  double *loc = work, *C = work + row, *dloc = C + cw * row, *dC = dloc + row, *rest = dC + cw * row;
  // a chain: the states and their tangents along gbar, the ping-pongs of w and dw, then the per-chunk partials
  double *states = nullptr, *tans = nullptr, *wpp = nullptr, *dwpp = nullptr, *part = rest;
  if (chain) states = rest, tans = states + (nl - 1) * row, wpp = tans + (nl - 1) * row, dwpp = wpp + 2 * row, part = dwpp + 2 * row;
  if (d_dinit && !chain) HIP_TRY(hipMemsetAsync(d_dinit, 0, sizeof(double) * row, st));
  // layer l at (h_l, t_l, w_{l+1}, dw_{l+1}).  mixed: only the last layer's iteration reaches the output, the earlier layers' sections
  // stay zero
  const double* cdw = nullptr;
  f64_walk_back(f, W, nl, h, gbar, h0, prb, states, tans, v, wpp, d_jtv, nullptr, st,
                [&](int l, bool end, const double* hl, const double* tl, const double* wl, double* dst) {
                  double* ddst = end ? d_dh : dwpp + (l & 1) * row;
                  jr_launch(f, W, nl, l, l == nl - 1, hl, tl, prb, nrm, wl, cdw, C, dloc, dC, part, d_grad, ddst, st);
                  if (d_dinit && !end) {   // ddst: the tangent of the cotangent on h_l, whose Dirichlet rows are h_initial's
                    PROF_BYTES(f->p->N * (1 + 16 * D));
                    LAUNCH("k_f64_pg_init", st,
                           (k_f64_pg_init<<<(unsigned)cdiv(row, 256), 256, 0, st>>>(f->p->N, f->p->flags, ddst, l != nl - 1, d_dinit)));
                  }
                  if (dst) vjp_launch(f, W, nl, l, l == nl - 1, hl, prb, nrm, wl, loc, C, nullptr, dst, nullptr, st);
                  cdw = ddst;
                });
  HIP_TRY(hipGetLastError());
  return PSIGNN_OK;
}

extern "C" int psignn_f64_vjp_backward(psignn_f64_t* f, const double* W, int nl, const double* h, const double* h0, const double* prb,
                                       const double* nrm, const double* v, const double* gbar, double* d_grad, double* d_dh,
                                       double* d_jtv, double* work, int64_t work_doubles, void* stream) {
  return vjp_backward_impl(__func__, f, W, nl, h, h0, prb, nrm, v, gbar, d_grad, d_dh, d_jtv, nullptr, work, work_doubles, stream);
}

extern "C" int psignn_f64_vjp_backward_init(psignn_f64_t* f, const double* W, int nl, const double* h, const double* h0,
                                            const double* prb, const double* nrm, const double* v, const double* gbar, double* d_grad,
                                            double* d_dh, double* d_jtv, double* d_dinit, double* work, int64_t work_doubles,
                                            void* stream) {
  return vjp_backward_impl(__func__, f, W, nl, h, h0, prb, nrm, v, gbar, d_grad, d_dh, d_jtv, d_dinit, work, work_doubles, stream);
}
