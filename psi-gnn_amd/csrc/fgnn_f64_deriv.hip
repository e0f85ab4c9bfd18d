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
// J v: one launch per layer gives the layer's value and its tangent together (k_f64_jvp_layer), so a multi-layer dirichlet chain
// stores no states.
// J^T w: two gather passes, no scatter.  An edge (r, c) sits once in r's CSR list and once in c's CSC list with the same attribute
// row, so what a scatter would add to the sending node is gathered there from the receiving nodes' records:
//   pass A (k_f64_vjp_node), per receiving node n: the node's forward again, w_n back through LayerNorm, gate and update (or
//          update_neumann), the node-local part of the result -- the x_i side of its own edges' messages included -- and the
//          cotangents of its message sums C[n] = {c_to, c_from (, c_neu)}, zero on Dirichlet rows;
//   pass B (k_f64_vjp_edge), per sending node m: over m's CSR entries the x_j side of Phi_to at the neighbour with the neighbour's
//          c_to, over m's CSC entries the x_j side of Phi_from with c_from (Neumann neighbours: Phi_neumann with c_neu); every ReLU
//          mask recomputed from h.  Optionally + a vector to add, which makes the map of the adjoint system y -> J^T y + grad one call.
// ReLU': 1 where the pre-activation is > 0 (torch's threshold_backward).
// Every kernel takes the done flag of a solver (NULL: none) and returns at once when it is set: psignn_f64_vjp_gated is the product of
// the float64 adjoint solves (solver_f64.hip, krylov_f64.hip), whose launches queued past the end of a solve or cycle change nothing.
#include "common.h"
#include "internal.h"
#include <math.h>

#if PSIGNN_D != 10
#error "fgnn_f64_deriv.hip is part of the default-width library only"
#endif

// The weight layout and the map handle of fgnn_f64.hip, repeated here token for token (that file is the pinned statement of the
// float64 forward and stays as it is): the same class defined the same way in two translation units.  tests/test_host_f64_deriv.py
// compares the two texts, so a field added there without being added here is a failing test, not a misread handle.
template <int P>
struct W64 {
  static constexpr int CAT = 3 * D + P, EIN = 2 * D + 3, NCAT = 2 * D + P + 2;
  static constexpr int LN_G = 0, LN_B = D, AL_W = 2 * D, AL_B = 2 * D + CAT, SHARED = 2 * D + CAT + 1;
  static constexpr int PHI_W1 = 0, PHI_B1 = D * EIN, PHI_W2 = D * EIN + D, PHI_B2 = D * EIN + D + D * D, PHI_SZ = D * EIN + 2 * D + D * D;
  static constexpr int UPD_B1 = D * CAT, UPD_W2 = D * CAT + D, UPD_B2 = D * CAT + D + D * D, UPD_SZ = D * CAT + 2 * D + D * D;
  static constexpr int NEU_B1 = D * NCAT, NEU_W2 = D * NCAT + D, NEU_B2 = D * NCAT + D + D * D, NEU_SZ = D * NCAT + 2 * D + D * D;
  static constexpr int LAYER = 2 * PHI_SZ + UPD_SZ;
  __host__ __device__ static constexpr int layer(int l) { return SHARED + l * LAYER; }
  __host__ __device__ static constexpr int total(int nl, bool mixed) { return SHARED + nl * LAYER + (mixed ? PHI_SZ + NEU_SZ : 0); }
};
static_assert(W64<2>::total(1, false) == 1193 && W64<3>::total(1, true) == 1924, "float64 weight layout at D = 10");

struct psignn_f64 {
  const psignn_plan* p = nullptr;   // borrowed: the plan outlives the handle
  double *csr_attr = nullptr, *csc_attr = nullptr;   // (Ep, 3) each, in the order of the plan's csr_nbr / csc_nbr
  double* pp[2] = {nullptr, nullptr};                // layer ping-pong of a multi-layer dirichlet block, made on first use
};

// ---------------------------------------------------------------------------------------------
// per edge
// ---------------------------------------------------------------------------------------------
// s = W1 [x_i; x_j; a] + b1, the pre-activations of one message (the order of fgnn_f64.hip's f64_message)
__device__ __forceinline__ void d64_pre(const double* __restrict__ Wp, const double* xi, const double* xj, const double* a, double* s) {
  using L = W64<2>;   // the Phi block has the same shape in both families
#pragma unroll
  for (int o = 0; o < D; ++o) {
    const double* w = Wp + L::PHI_W1 + o * L::EIN;
    double t = Wp[L::PHI_B1 + o];
#pragma unroll
    for (int k = 0; k < D; ++k) t = fma(w[k], xi[k], t);
#pragma unroll
    for (int k = 0; k < D; ++k) t = fma(w[D + k], xj[k], t);
#pragma unroll
    for (int k = 0; k < 3; ++k) t = fma(w[2 * D + k], a[k], t);
    s[o] = t;
  }
}
__device__ __forceinline__ void d64_row(const double* __restrict__ h, int64_t u, double* x) {
#pragma unroll
  for (int k = 0; k < D; ++k) x[k] = h[u * D + k];
}
// q = W2^T c: the cotangent of a message's hidden layer before the ReLU mask
__device__ __forceinline__ void d64_w2t(const double* __restrict__ Wp, const double* c, double* q) {
  using L = W64<2>;
#pragma unroll
  for (int k = 0; k < D; ++k) q[k] = 0.0;
#pragma unroll
  for (int o = 0; o < D; ++o)
#pragma unroll
    for (int k = 0; k < D; ++k) q[k] = fma(Wp[L::PHI_W2 + o * D + k], c[o], q[k]);
}

// Sum of the messages of one Phi module over one edge list of node n, and (TAN) of their tangents along (dx, v):
// d message = W2 (1[s > 0] * (W1_i dx + W1_j v_u)).
template <bool TAN>
__device__ __forceinline__ void d64_phi(const double* __restrict__ Wp, const double* x, const double* dx, const double* __restrict__ h,
                                        const double* __restrict__ v, int32_t beg, int32_t end, const int32_t* __restrict__ nbr,
                                        const double* __restrict__ attr, double* mp, double* dmp) {
  using L = W64<2>;
#pragma unroll
  for (int o = 0; o < D; ++o) {
    mp[o] = 0.0;
    if (TAN) dmp[o] = 0.0;
  }
  for (int32_t i = beg; i < end; ++i) {
    const int64_t u = nbr[i];
    double xj[D], a[3], s[D], t[D];
    d64_row(h, u, xj);
#pragma unroll
    for (int k = 0; k < 3; ++k) a[k] = attr[3 * (int64_t)i + k];
    d64_pre(Wp, x, xj, a, s);
    if (TAN) {
      double dxj[D];
      d64_row(v, u, dxj);
#pragma unroll
      for (int o = 0; o < D; ++o) {
        const double* w = Wp + L::PHI_W1 + o * L::EIN;
        double r = 0.0;
#pragma unroll
        for (int k = 0; k < D; ++k) r = fma(w[k], dx[k], r);
#pragma unroll
        for (int k = 0; k < D; ++k) r = fma(w[D + k], dxj[k], r);
        t[o] = s[o] > 0.0 ? r : 0.0;
      }
    }
#pragma unroll
    for (int o = 0; o < D; ++o) s[o] = fmax(s[o], 0.0);
#pragma unroll
    for (int o = 0; o < D; ++o) {
      const double* w = Wp + L::PHI_W2 + o * D;
      double r = Wp[L::PHI_B2 + o];
#pragma unroll
      for (int k = 0; k < D; ++k) r = fma(w[k], s[k], r);
      mp[o] += r;
      if (TAN) {
        double dr = 0.0;
#pragma unroll
        for (int k = 0; k < D; ++k) dr = fma(w[k], t[k], dr);
        dmp[o] += dr;
      }
    }
  }
}

// x_i side of the messages node n receives over one edge list: gx += sum_e W1_i^T (1[s_e > 0] * q), q = W2^T c of the node
__device__ __forceinline__ void d64_phi_vjp_xi(const double* __restrict__ Wp, const double* x, const double* __restrict__ h, int32_t beg,
                                               int32_t end, const int32_t* __restrict__ nbr, const double* __restrict__ attr,
                                               const double* q, double* gx) {
  using L = W64<2>;
  for (int32_t i = beg; i < end; ++i) {
    double xj[D], a[3], s[D];
    d64_row(h, nbr[i], xj);
#pragma unroll
    for (int k = 0; k < 3; ++k) a[k] = attr[3 * (int64_t)i + k];
    d64_pre(Wp, x, xj, a, s);
#pragma unroll
    for (int o = 0; o < D; ++o) {
      const double r = s[o] > 0.0 ? q[o] : 0.0;
#pragma unroll
      for (int k = 0; k < D; ++k) gx[k] = fma(Wp[L::PHI_W1 + o * L::EIN + k], r, gx[k]);
    }
  }
}

// x_j side of ONE message that neighbour u receives from node m (x = h[m]) with u's cotangent c: g += W1_j^T (1[s > 0] * W2^T c)
__device__ __forceinline__ void d64_msg_vjp_xj(const double* __restrict__ Wp, const double* xu, const double* x, const double* a,
                                               const double* c, double* g) {
  using L = W64<2>;
  double s[D], q[D];
  d64_pre(Wp, xu, x, a, s);
  d64_w2t(Wp, c, q);
#pragma unroll
  for (int o = 0; o < D; ++o) {
    const double r = s[o] > 0.0 ? q[o] : 0.0;
#pragma unroll
    for (int k = 0; k < D; ++k) g[k] = fma(Wp[L::PHI_W1 + o * L::EIN + D + k], r, g[k]);
  }
}

// LayerNorm(10), eps 1e-5, biased variance (model.py:293): statistics of y; yhat = (y - mu) * rs
__device__ __forceinline__ double d64_ln_stats(const double* y, double* yhat) {
  double mu = 0.0;
#pragma unroll
  for (int o = 0; o < D; ++o) mu += y[o];
  mu /= D;
  double var = 0.0;
#pragma unroll
  for (int o = 0; o < D; ++o) var = fma(y[o] - mu, y[o] - mu, var);
  var /= D;
  const double rs = 1.0 / sqrt(var + 1e-5);
#pragma unroll
  for (int o = 0; o < D; ++o) yhat[o] = (y[o] - mu) * rs;
  return rs;
}

// ---------------------------------------------------------------------------------------------
// J v: one layer, one node per lane.  out_h (may be NULL): the layer's value; out_v: its tangent (TAN).  TAN = false is the plain
// layer (the states of a multi-layer J^T w).  lofs / nofs: as k_f64_layer.
// ---------------------------------------------------------------------------------------------
template <int P, bool MIXED, bool TAN>
__global__ __launch_bounds__(256) void k_f64_jvp_layer(int64_t N, const double* __restrict__ W, int lofs, int nofs, int apply_ln,
                                                       const int32_t* __restrict__ csr_ptr, const int32_t* __restrict__ csr_nbr,
                                                       const double* __restrict__ csr_attr, const int32_t* __restrict__ csc_ptr,
                                                       const int32_t* __restrict__ csc_nbr, const double* __restrict__ csc_attr,
                                                       const uint8_t* __restrict__ flags, const double* __restrict__ h,
                                                       const double* __restrict__ v, const double* __restrict__ h0,
                                                       const double* __restrict__ prb, const double* __restrict__ nrm,
                                                       double* __restrict__ out_h, double* __restrict__ out_v,
                                                       const int32_t* __restrict__ done) {
  using L = W64<P>;
  if (done && *done) return;
  const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  const uint8_t fl = flags[n];
  if (fl & FLAG_DIRICHLET) {   // the row is h_initial's: tangent 0
#pragma unroll
    for (int o = 0; o < D; ++o) {
      if (out_h) out_h[n * D + o] = h0[n * D + o];
      if (TAN) out_v[n * D + o] = 0.0;
    }
    return;
  }
  double x[D], dx[D], y[D], dy[D];
  d64_row(h, n, x);
  if (TAN) d64_row(v, n, dx);
  const int32_t rb = csr_ptr[n], re = csr_ptr[n + 1];
  if (MIXED && (fl & FLAG_NEUMANN)) {
    double mp[D], dmp[D], cat[L::NCAT], hid[D], dhid[D];
    d64_phi<TAN>(W + nofs, x, dx, h, v, rb, re, csr_nbr, csr_attr, mp, dmp);
#pragma unroll
    for (int k = 0; k < D; ++k) {
      cat[k] = x[k];
      cat[D + k] = mp[k];
    }
#pragma unroll
    for (int k = 0; k < P; ++k) cat[2 * D + k] = prb[n * P + k];
    cat[2 * D + P] = nrm[2 * n];
    cat[2 * D + P + 1] = nrm[2 * n + 1];
    const double* Wn = W + nofs + L::PHI_SZ;
#pragma unroll
    for (int o = 0; o < D; ++o) {
      double s = Wn[L::NEU_B1 + o];
#pragma unroll
      for (int k = 0; k < L::NCAT; ++k) s = fma(Wn[o * L::NCAT + k], cat[k], s);
      if (TAN) {
        double r = 0.0;
#pragma unroll
        for (int k = 0; k < D; ++k) r = fma(Wn[o * L::NCAT + k], dx[k], r);
#pragma unroll
        for (int k = 0; k < D; ++k) r = fma(Wn[o * L::NCAT + D + k], dmp[k], r);
        dhid[o] = s > 0.0 ? r : 0.0;
      }
      hid[o] = fmax(s, 0.0);
    }
#pragma unroll
    for (int o = 0; o < D; ++o) {
      double s = Wn[L::NEU_B2 + o], r = 0.0;
#pragma unroll
      for (int k = 0; k < D; ++k) s = fma(Wn[L::NEU_W2 + o * D + k], hid[k], s);
      y[o] = s;
      if (TAN) {
#pragma unroll
        for (int k = 0; k < D; ++k) r = fma(Wn[L::NEU_W2 + o * D + k], dhid[k], r);
        dy[o] = r;
      }
    }
  } else {
    double cat[L::CAT], dcat[3 * D], hid[D], dhid[D];
#pragma unroll
    for (int k = 0; k < D; ++k) {
      cat[k] = x[k];
      if (TAN) dcat[k] = dx[k];
    }
    d64_phi<TAN>(W + lofs, x, dx, h, v, csc_ptr[n], csc_ptr[n + 1], csc_nbr, csc_attr, cat + D, dcat + D);
    d64_phi<TAN>(W + lofs + L::PHI_SZ, x, dx, h, v, rb, re, csr_nbr, csr_attr, cat + 2 * D, dcat + 2 * D);
#pragma unroll
    for (int k = 0; k < P; ++k) cat[3 * D + k] = prb[n * P + k];
    double al = W[L::AL_B], dal = 0.0;
#pragma unroll
    for (int k = 0; k < L::CAT; ++k) al = fma(W[L::AL_W + k], cat[k], al);
    al = 1.0 / (1.0 + exp(-al));
    if (TAN) {
#pragma unroll
      for (int k = 0; k < 3 * D; ++k) dal = fma(W[L::AL_W + k], dcat[k], dal);
      dal *= al * (1.0 - al);
    }
    const double* Wu = W + lofs + 2 * L::PHI_SZ;
#pragma unroll
    for (int o = 0; o < D; ++o) {
      double s = Wu[L::UPD_B1 + o];
#pragma unroll
      for (int k = 0; k < L::CAT; ++k) s = fma(Wu[o * L::CAT + k], cat[k], s);
      if (TAN) {
        double r = 0.0;
#pragma unroll
        for (int k = 0; k < 3 * D; ++k) r = fma(Wu[o * L::CAT + k], dcat[k], r);
        dhid[o] = s > 0.0 ? r : 0.0;
      }
      hid[o] = fmax(s, 0.0);
    }
#pragma unroll
    for (int o = 0; o < D; ++o) {
      double s = Wu[L::UPD_B2 + o], r = 0.0;
#pragma unroll
      for (int k = 0; k < D; ++k) s = fma(Wu[L::UPD_W2 + o * D + k], hid[k], s);
      y[o] = x[o] + al * s;
      if (TAN) {
#pragma unroll
        for (int k = 0; k < D; ++k) r = fma(Wu[L::UPD_W2 + o * D + k], dhid[k], r);
        dy[o] = dx[o] + dal * s + al * r;
      }
    }
  }
  if (apply_ln) {
    double yhat[D];
    const double rs = d64_ln_stats(y, yhat);
    if (TAN) {   // d yhat = rs (dyc - yhat mean(yhat dyc)), dyc = dy - mean(dy)
      double m1 = 0.0, m2 = 0.0;
#pragma unroll
      for (int o = 0; o < D; ++o) m1 += dy[o];
      m1 /= D;
#pragma unroll
      for (int o = 0; o < D; ++o) m2 = fma(yhat[o], dy[o] - m1, m2);
      m2 /= D;
#pragma unroll
      for (int o = 0; o < D; ++o) dy[o] = rs * ((dy[o] - m1) - yhat[o] * m2) * W[L::LN_G + o];
    }
#pragma unroll
    for (int o = 0; o < D; ++o) y[o] = yhat[o] * W[L::LN_G + o] + W[L::LN_B + o];
  }
#pragma unroll
  for (int o = 0; o < D; ++o) {
    if (out_h) out_h[n * D + o] = y[o];
    if (TAN) out_v[n * D + o] = dy[o];
  }
}

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
  double gx[D], c[CW];
#pragma unroll
  for (int k = 0; k < D; ++k) gx[k] = 0.0;
#pragma unroll
  for (int k = 0; k < CW; ++k) c[k] = 0.0;
  if (!(fl & FLAG_DIRICHLET)) {   // a Dirichlet row is h_initial's: nothing flows back through it
    double x[D], gy[D];
    d64_row(h, n, x);
    d64_row(w, n, gy);
    const int32_t rb = csr_ptr[n], re = csr_ptr[n + 1], cb = csc_ptr[n], ce = csc_ptr[n + 1];
    if (MIXED && (fl & FLAG_NEUMANN)) {
      double mp[D], cat[L::NCAT], pre[D], y[D], q[D];
      d64_phi<false>(W + nofs, x, nullptr, h, nullptr, rb, re, csr_nbr, csr_attr, mp, nullptr);
#pragma unroll
      for (int k = 0; k < D; ++k) {
        cat[k] = x[k];
        cat[D + k] = mp[k];
      }
#pragma unroll
      for (int k = 0; k < P; ++k) cat[2 * D + k] = prb[n * P + k];
      cat[2 * D + P] = nrm[2 * n];
      cat[2 * D + P + 1] = nrm[2 * n + 1];
      const double* Wn = W + nofs + L::PHI_SZ;
#pragma unroll
      for (int o = 0; o < D; ++o) {
        double s = Wn[L::NEU_B1 + o];
#pragma unroll
        for (int k = 0; k < L::NCAT; ++k) s = fma(Wn[o * L::NCAT + k], cat[k], s);
        pre[o] = s;
      }
      if (apply_ln) {
#pragma unroll
        for (int o = 0; o < D; ++o) {
          double s = Wn[L::NEU_B2 + o];
#pragma unroll
          for (int k = 0; k < D; ++k) s = fma(Wn[L::NEU_W2 + o * D + k], fmax(pre[k], 0.0), s);
          y[o] = s;
        }
        double yhat[D], m1 = 0.0, m2 = 0.0;
        const double rs = d64_ln_stats(y, yhat);
#pragma unroll
        for (int o = 0; o < D; ++o) {
          gy[o] *= W[L::LN_G + o];
          m1 += gy[o];
          m2 = fma(gy[o], yhat[o], m2);
        }
        m1 /= D;
        m2 /= D;
#pragma unroll
        for (int o = 0; o < D; ++o) gy[o] = rs * (gy[o] - m1 - yhat[o] * m2);
      }
      // y = N2 relu(N1 cat + n1) + n2
#pragma unroll
      for (int k = 0; k < D; ++k) {
        double s = 0.0;
#pragma unroll
        for (int o = 0; o < D; ++o) s = fma(Wn[L::NEU_W2 + o * D + k], gy[o], s);
        q[k] = pre[k] > 0.0 ? s : 0.0;
      }
#pragma unroll
      for (int o = 0; o < D; ++o)
#pragma unroll
        for (int k = 0; k < D; ++k) {
          gx[k] = fma(Wn[o * L::NCAT + k], q[o], gx[k]);
          c[2 * D + k] = fma(Wn[o * L::NCAT + D + k], q[o], c[2 * D + k]);
        }
      d64_w2t(W + nofs, c + 2 * D, q);
      d64_phi_vjp_xi(W + nofs, x, h, rb, re, csr_nbr, csr_attr, q, gx);
    } else {
      double cat[L::CAT], pre[D], sv[D], y[D], gcat[3 * D], q[D];
#pragma unroll
      for (int k = 0; k < D; ++k) cat[k] = x[k];
      d64_phi<false>(W + lofs, x, nullptr, h, nullptr, cb, ce, csc_nbr, csc_attr, cat + D, nullptr);
      d64_phi<false>(W + lofs + L::PHI_SZ, x, nullptr, h, nullptr, rb, re, csr_nbr, csr_attr, cat + 2 * D, nullptr);
#pragma unroll
      for (int k = 0; k < P; ++k) cat[3 * D + k] = prb[n * P + k];
      double al = W[L::AL_B];
#pragma unroll
      for (int k = 0; k < L::CAT; ++k) al = fma(W[L::AL_W + k], cat[k], al);
      al = 1.0 / (1.0 + exp(-al));
      const double* Wu = W + lofs + 2 * L::PHI_SZ;
#pragma unroll
      for (int o = 0; o < D; ++o) {
        double s = Wu[L::UPD_B1 + o];
#pragma unroll
        for (int k = 0; k < L::CAT; ++k) s = fma(Wu[o * L::CAT + k], cat[k], s);
        pre[o] = s;
      }
#pragma unroll
      for (int o = 0; o < D; ++o) {
        double s = Wu[L::UPD_B2 + o];
#pragma unroll
        for (int k = 0; k < D; ++k) s = fma(Wu[L::UPD_W2 + o * D + k], fmax(pre[k], 0.0), s);
        sv[o] = s;
        y[o] = x[o] + al * s;
      }
      if (apply_ln) {
        double yhat[D], m1 = 0.0, m2 = 0.0;
        const double rs = d64_ln_stats(y, yhat);
#pragma unroll
        for (int o = 0; o < D; ++o) {
          gy[o] *= W[L::LN_G + o];
          m1 += gy[o];
          m2 = fma(gy[o], yhat[o], m2);
        }
        m1 /= D;
        m2 /= D;
#pragma unroll
        for (int o = 0; o < D; ++o) gy[o] = rs * (gy[o] - m1 - yhat[o] * m2);
      }
      // y = x + al * s: cotangents of the gate's pre-activation and of s
      double gal = 0.0;
#pragma unroll
      for (int o = 0; o < D; ++o) gal = fma(gy[o], sv[o], gal);
      gal *= al * (1.0 - al);
#pragma unroll
      for (int k = 0; k < 3 * D; ++k) gcat[k] = W[L::AL_W + k] * gal;
#pragma unroll
      for (int k = 0; k < D; ++k) {
        double s = 0.0;
#pragma unroll
        for (int o = 0; o < D; ++o) s = fma(Wu[L::UPD_W2 + o * D + k], al * gy[o], s);
        q[k] = pre[k] > 0.0 ? s : 0.0;
      }
#pragma unroll
      for (int o = 0; o < D; ++o)
#pragma unroll
        for (int k = 0; k < 3 * D; ++k) gcat[k] = fma(Wu[o * L::CAT + k], q[o], gcat[k]);
#pragma unroll
      for (int k = 0; k < D; ++k) {
        gx[k] = gy[k] + gcat[k];
        c[k] = gcat[D + k];
        c[D + k] = gcat[2 * D + k];
      }
      d64_w2t(W + lofs, c, q);
      d64_phi_vjp_xi(W + lofs, x, h, cb, ce, csc_nbr, csc_attr, q, gx);
      d64_w2t(W + lofs + L::PHI_SZ, c + D, q);
      d64_phi_vjp_xi(W + lofs + L::PHI_SZ, x, h, rb, re, csr_nbr, csr_attr, q, gx);
    }
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
#define F64_EDGES(f) (f)->p->csr_ptr, (f)->p->csr_nbr, (f)->csr_attr, (f)->p->csc_ptr, (f)->p->csc_nbr, (f)->csc_attr, (f)->p->flags

// one layer's value (out_h, may be NULL) and, with v, its tangent (out_v)
static void jvp_launch(const psignn_f64* f, const double* W, int nl, int l, int apply_ln, const double* h, const double* v,
                       const double* h0, const double* prb, const double* nrm, double* out_h, double* out_v, const int32_t* done,
                       hipStream_t st) {
  const psignn_plan* p = f->p;
  const unsigned g = (unsigned)cdiv(p->N, 256);
  // algorithmic bytes: both edge lists once (neighbour id, 3 attributes, the neighbour's row and tangent row), per node its rows
  PROF_BYTES(2 * p->Ep * (4 + 24 + (v ? 16 : 8) * D) + p->N * ((v ? 32 : 16) * D + 8 * (p->mixed ? 3 : 2) + 17));
  if (p->mixed) {
    using L = W64<3>;
    LAUNCH("k_f64_jvp_layer", st,
           (k_f64_jvp_layer<3, true, true><<<g, 256, 0, st>>>(p->N, W, L::layer(l), L::layer(nl), apply_ln, F64_EDGES(f), h, v, h0, prb,
                                                             nrm, out_h, out_v, done)));
  } else if (v) {
    using L = W64<2>;
    LAUNCH("k_f64_jvp_layer", st,
           (k_f64_jvp_layer<2, false, true><<<g, 256, 0, st>>>(p->N, W, L::layer(l), L::layer(nl), apply_ln, F64_EDGES(f), h, v, h0,
                                                              prb, nrm, out_h, out_v, done)));
  } else {
    using L = W64<2>;
    LAUNCH("k_f64_state_layer", st,
           (k_f64_jvp_layer<2, false, false><<<g, 256, 0, st>>>(p->N, W, L::layer(l), L::layer(nl), apply_ln, F64_EDGES(f), h, nullptr,
                                                               h0, prb, nrm, out_h, nullptr, done)));
  }
}

// both passes of one layer: out = J_l(h)^T w (+ add)
static void vjp_launch(const psignn_f64* f, const double* W, int nl, int l, int apply_ln, const double* h, const double* prb,
                       const double* nrm, const double* w, double* loc, double* C, const double* add, double* out, const int32_t* done,
                       hipStream_t st) {
  const psignn_plan* p = f->p;
  const unsigned g = (unsigned)cdiv(p->N, 256);
  const int cw = p->mixed ? 3 * D : 2 * D;
  PROF_BYTES(2 * p->Ep * (4 + 24 + 8 * D) + p->N * (8 * (3 * D + cw) + 8 * (p->mixed ? 3 : 2) + 17));
  if (p->mixed) {
    using L = W64<3>;
    LAUNCH("k_f64_vjp_node", st,
           (k_f64_vjp_node<3, true><<<g, 256, 0, st>>>(p->N, W, L::layer(l), L::layer(nl), apply_ln, F64_EDGES(f), h, prb, nrm, w, loc,
                                                      C, done)));
  } else {
    using L = W64<2>;
    LAUNCH("k_f64_vjp_node", st,
           (k_f64_vjp_node<2, false><<<g, 256, 0, st>>>(p->N, W, L::layer(l), L::layer(nl), apply_ln, F64_EDGES(f), h, prb, nrm, w, loc,
                                                       C, done)));
  }
  // both edge lists once (neighbour id and flag, 3 attributes, the neighbour's row and its cotangent), per node h, loc, out (, add)
  PROF_BYTES(2 * p->Ep * (4 + 1 + 24 + 16 * D) + p->N * (8 * 3 * D + (add ? 8 * D : 0) + 8));
  if (p->mixed) {
    using L = W64<3>;
    LAUNCH("k_f64_vjp_edge", st,
           (k_f64_vjp_edge<true><<<g, 256, 0, st>>>(p->N, W, L::layer(l), L::layer(nl), F64_EDGES(f), h, loc, C, add, out, done)));
  } else {
    using L = W64<2>;
    LAUNCH("k_f64_vjp_edge", st,
           (k_f64_vjp_edge<false><<<g, 256, 0, st>>>(p->N, W, L::layer(l), L::layer(nl), F64_EDGES(f), h, loc, C, add, out, done)));
  }
}

// Only a multi-layer dirichlet block is a chain: the mixed loop never reassigns h, so its last layer on h is the block.
static inline bool f64_chain(const psignn_f64* f, int nl) { return !f->p->mixed && nl > 1; }

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

extern "C" int psignn_f64_jvp(psignn_f64_t* f, const double* W, int nl, const double* h, const double* h0, const double* prb,
                              const double* nrm, const double* v, double* out, double* work, int64_t work_doubles, void* stream) {
  ARG_CHECK(f && W && h && h0 && prb && v && out, "NULL argument");
  ARG_CHECK(nl >= 1 && nl <= 64, "n_layers out of range");
  ARG_CHECK(!f->p->mixed || nrm, "mixed plan needs unit normals");
  ARG_CHECK(out != h && out != v, "out must not alias h or v");
  const int rc = work_check(__func__, psignn_f64_deriv_workspace_doubles(f, nl, 0), work, work_doubles);
  if (rc) return rc;
  if (f->p->N == 0) return PSIGNN_OK;
  hipStream_t st = (hipStream_t)stream;
  if (!f64_chain(f, nl)) {
    jvp_launch(f, W, nl, nl - 1, 1, h, v, h0, prb, nrm, nullptr, out, nullptr, st);
  } else {
    const int64_t row = f->p->N * D;
    const double *ch = h, *cv = v;
    for (int l = 0; l < nl; ++l) {
      const bool last = l == nl - 1;
      double* dh = last ? nullptr : work + (l & 1) * row;
      double* dv = last ? out : work + (2 + (l & 1)) * row;
      jvp_launch(f, W, nl, l, last, ch, cv, h0, prb, nrm, dh, dv, nullptr, st);
      ch = dh;
      cv = dv;
    }
  }
  HIP_TRY(hipGetLastError());
  return PSIGNN_OK;
}

// The product with the flag of a solver (internal.h): every launch returns at once when *done is set (NULL: no flag).
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
  double *loc = work, *C = work + row;
  if (!f64_chain(f, nl)) {
    vjp_launch(f, W, nl, nl - 1, 1, h, prb, nrm, w, loc, C, add, out, done, st);
  } else {
    // the states h_1 .. h_{L-1} at h, then the chain backwards; cotangents of the inner layers in a ping-pong
    double *states = work + 3 * row, *pp = work + (3 + nl - 1) * row;
    const double* cur = h;
    for (int l = 0; l + 1 < nl; ++l) {
      jvp_launch(f, W, nl, l, 0, cur, nullptr, h0, prb, nullptr, states + l * row, nullptr, done, st);
      cur = states + l * row;
    }
    const double* cw = w;
    for (int l = nl - 1; l >= 0; --l) {
      double* dst = l == 0 ? out : pp + (l & 1) * row;
      vjp_launch(f, W, nl, l, l == nl - 1, l == 0 ? h : states + (l - 1) * row, prb, nrm, cw, loc, C, l == 0 ? add : nullptr, dst,
                 done, st);
      cw = dst;
    }
  }
  HIP_TRY(hipGetLastError());
  return PSIGNN_OK;
}

extern "C" int psignn_f64_vjp(psignn_f64_t* f, const double* W, int nl, const double* h, const double* h0, const double* prb,
                              const double* nrm, const double* w, const double* add, double* out, double* work,
                              int64_t work_doubles, void* stream) {
  return psignn_f64_vjp_gated(f, W, nl, h, h0, prb, nrm, w, add, out, work, work_doubles, nullptr, (hipStream_t)stream);
}
