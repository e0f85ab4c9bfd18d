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
// The weight layout W64 and the map handle psignn_f64 are those of fgnn_f64.hip: both files take them from f64_common.h.
#include "f64_common.h"
#include <math.h>

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
// gy, the cotangent of LayerNorm's output at y, back through it: gy <- rs (g - mean(g) - yhat mean(g yhat)), g = gamma * gy
__device__ __forceinline__ void d64_ln_back(const double* __restrict__ gamma, const double* y, double* gy) {
  double yhat[D], m1 = 0.0, m2 = 0.0;
  const double rs = d64_ln_stats(y, yhat);
#pragma unroll
  for (int o = 0; o < D; ++o) {
    gy[o] *= gamma[o];
    m1 += gy[o];
    m2 = fma(gy[o], yhat[o], m2);
  }
  m1 /= D;
  m2 /= D;
#pragma unroll
  for (int o = 0; o < D; ++o) gy[o] = rs * (gy[o] - m1 - yhat[o] * m2);
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
        d64_ln_back(W + L::LN_G, y, gy);
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
      if (apply_ln) d64_ln_back(W + L::LN_G, y, gy);
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
__device__ __forceinline__ void pg_edges(const double* __restrict__ Wp, bool act, const double* x, const double* c,
                                         const double* __restrict__ h, int32_t beg, int32_t end, const int32_t* __restrict__ nbr,
                                         const double* __restrict__ attr, double* buf, double* row, double* pt, int base) {
  using L = W64<2>;
  double q[D], a1[2] = {0.0, 0.0}, a2[1] = {0.0};
  d64_w2t(Wp, c, q);
  for (int32_t j = 0;; ++j) {
    const bool on = act && beg + j < end;
    if (!__syncthreads_or(on)) break;   // also the barrier behind the previous round's reads
    if (on) {
      const int32_t i = beg + j;
      double xj[D], a[3], s[D];
      d64_row(h, nbr[i], xj);
#pragma unroll
      for (int k = 0; k < 3; ++k) a[k] = attr[3 * (int64_t)i + k];
      d64_pre(Wp, x, xj, a, s);
#pragma unroll
      for (int k = 0; k < D; ++k) {
        row[k] = s[k] > 0.0 ? q[k] : 0.0;
        row[10 + k] = x[k];
        row[20 + k] = xj[k];
        row[34 + k] = c[k];
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
  }
  pg_put<2>(pt, base + L::PHI_W1, base + L::PHI_B1, D, L::EIN + 1, a1);
  pg_put<1>(pt, base + L::PHI_W2, base + L::PHI_B2, D, D + 1, a2);
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
  constexpr int CW = MIXED ? 3 * D : 2 * D;
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
  double x[D], c[CW], q[D], cat[L::CAT], g[D], rp[D], wy[D], gw[D], gal = 0.0;
  int32_t rb = 0, re = 0, cb = 0, ce = 0;
#pragma unroll
  for (int k = 0; k < D; ++k) x[k] = q[k] = g[k] = rp[k] = wy[k] = gw[k] = 0.0;
#pragma unroll
  for (int k = 0; k < CW; ++k) c[k] = 0.0;
#pragma unroll
  for (int k = 0; k < L::CAT; ++k) cat[k] = 0.0;
  if (live) {
    double gy[D], pre[D], y[D];
    d64_row(h, n, x);
    d64_row(w, n, gy);
    rb = csr_ptr[n], re = csr_ptr[n + 1], cb = csc_ptr[n], ce = csc_ptr[n + 1];
    double al = 1.0;
    const double* Wm = neu ? W + nofs + L::PHI_SZ : W + lofs + 2 * L::PHI_SZ;   // W1 | b1 | W2 | b2 of the row's MLP
    int ncat, ob1, ow2, ob2;
    if (neu) {
      double mp[D];
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
      ncat = L::NCAT, ob1 = L::NEU_B1, ow2 = L::NEU_W2, ob2 = L::NEU_B2;
    } else {
#pragma unroll
      for (int k = 0; k < D; ++k) cat[k] = x[k];
      d64_phi<false>(W + lofs, x, nullptr, h, nullptr, cb, ce, csc_nbr, csc_attr, cat + D, nullptr);
      d64_phi<false>(W + lofs + L::PHI_SZ, x, nullptr, h, nullptr, rb, re, csr_nbr, csr_attr, cat + 2 * D, nullptr);
#pragma unroll
      for (int k = 0; k < P; ++k) cat[3 * D + k] = prb[n * P + k];
      al = W[L::AL_B];
#pragma unroll
      for (int k = 0; k < L::CAT; ++k) al = fma(W[L::AL_W + k], cat[k], al);
      al = 1.0 / (1.0 + exp(-al));
      ncat = L::CAT, ob1 = L::UPD_B1, ow2 = L::UPD_W2, ob2 = L::UPD_B2;
    }
#pragma unroll
    for (int o = 0; o < D; ++o) {
      double s = Wm[ob1 + o];
#pragma unroll
      for (int k = 0; k < L::CAT; ++k)
        if (k < ncat) s = fma(Wm[o * ncat + k], cat[k], s);
      pre[o] = s;
      rp[o] = fmax(s, 0.0);
    }
    double sv[D];
#pragma unroll
    for (int o = 0; o < D; ++o) {
      double s = Wm[ob2 + o];
#pragma unroll
      for (int k = 0; k < D; ++k) s = fma(Wm[ow2 + o * D + k], rp[k], s);
      sv[o] = s;
      y[o] = neu ? s : x[o] + al * s;
    }
    if (apply_ln) {
      double yhat[D], m1 = 0.0, m2 = 0.0;
      const double rs = d64_ln_stats(y, yhat);
#pragma unroll
      for (int o = 0; o < D; ++o) {
        wy[o] = gy[o] * yhat[o];
        gw[o] = gy[o];
        gy[o] *= W[L::LN_G + o];
        m1 += gy[o];
        m2 = fma(gy[o], yhat[o], m2);
      }
      m1 /= D;
      m2 /= D;
#pragma unroll
      for (int o = 0; o < D; ++o) gy[o] = rs * (gy[o] - m1 - yhat[o] * m2);
    }
    if (!neu) {   // y = x + al * s: cotangent of the gate's pre-activation
#pragma unroll
      for (int o = 0; o < D; ++o) gal = fma(gy[o], sv[o], gal);
      gal *= al * (1.0 - al);
    }
#pragma unroll
    for (int o = 0; o < D; ++o) g[o] = al * gy[o];
#pragma unroll
    for (int k = 0; k < D; ++k) {
      double s = 0.0;
#pragma unroll
      for (int o = 0; o < D; ++o) s = fma(Wm[ow2 + o * D + k], g[o], s);
      q[k] = pre[k] > 0.0 ? s : 0.0;
    }
    // cotangents of the message sums: cat[D .. 2D) (and [2D .. 3D) of an update row)
    if (neu) {
#pragma unroll
      for (int k = 0; k < D; ++k) {
        double s = 0.0;
#pragma unroll
        for (int o = 0; o < D; ++o) s = fma(Wm[o * L::NCAT + D + k], q[o], s);
        c[CW - D + k] = s;
      }
    } else {
#pragma unroll
      for (int k = 0; k < 2 * D; ++k) {
        double s = W[L::AL_W + D + k] * gal;
#pragma unroll
        for (int o = 0; o < D; ++o) s = fma(Wm[o * L::CAT + D + k], q[o], s);
        c[k] = s;
      }
    }
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
  pg_edges(W + lofs, upd, x, c, h, cb, ce, csc_nbr, csc_attr, buf, row, pt, L::layer(0));
  pg_edges(W + lofs + L::PHI_SZ, upd, x, c + D, h, rb, re, csr_nbr, csr_attr, buf, row, pt, L::layer(0) + L::PHI_SZ);
  if (MIXED) pg_edges(W + nofs, neu, x, c + 2 * D, h, rb, re, csr_nbr, csr_attr, buf, row, pt, L::layer(1));
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
  if (p->mixed) {
    using L = W64<3>;
    LAUNCH("k_f64_pgrad", st,
           (k_f64_pgrad<3, true><<<(unsigned)nch, PG_ROWS, 0, st>>>(p->N, W, L::layer(l), L::layer(nl), apply_ln, F64_EDGES(f), h, prb,
                                                                    nrm, w, part)));
    pg_reduce(part, nch, L::total(1, true), L::SHARED, L::LAYER, L::layer(l), L::layer(nl), grad, st);
  } else {
    using L = W64<2>;
    LAUNCH("k_f64_pgrad", st,
           (k_f64_pgrad<2, false><<<(unsigned)nch, PG_ROWS, 0, st>>>(p->N, W, L::layer(l), L::layer(nl), apply_ln, F64_EDGES(f), h, prb,
                                                                     nrm, w, part)));
    pg_reduce(part, nch, L::total(1, false), L::SHARED, L::LAYER, L::layer(l), L::layer(nl), grad, st);
  }
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
  if (!f64_chain(f, nl)) {   // mixed: only the last layer's iteration reaches the output, the earlier layers' sections stay zero
    pgrad_launch(f, W, nl, nl - 1, 1, h, prb, nrm, w, part, d_grad, d_out_init, 0, st);
    vjp_launch(f, W, nl, nl - 1, 1, h, prb, nrm, w, loc, C, nullptr, d_out_h, nullptr, st);
  } else {
    // as psignn_f64_vjp: the states, then the chain backwards; layer l's gradient at (h_l, w_{l+1}) before w_l = J_l^T w_{l+1}
    double *states = work + 3 * row, *pp = work + (3 + nl - 1) * row;
    const double* cur = h;
    for (int l = 0; l + 1 < nl; ++l) {
      jvp_launch(f, W, nl, l, 0, cur, nullptr, h0, prb, nullptr, states + l * row, nullptr, nullptr, st);
      cur = states + l * row;
    }
    const double* cw = w;
    for (int l = nl - 1; l >= 0; --l) {
      const double* hl = l == 0 ? h : states + (l - 1) * row;
      double* dst = l == 0 ? d_out_h : pp + (l & 1) * row;
      pgrad_launch(f, W, nl, l, l == nl - 1, hl, prb, nrm, cw, part, d_grad, d_out_init, l != nl - 1, st);
      vjp_launch(f, W, nl, l, l == nl - 1, hl, prb, nrm, cw, loc, C, nullptr, dst, nullptr, st);
      cw = dst;
    }
  }
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
// d64_ln_back with its tangent along dy: (gy, dgy) the cotangent of LayerNorm's output and its tangent, back through it at y.
// yhat, dyh: the normalised row and its tangent (the factors of laynorm.weight's gradient).
__device__ __forceinline__ void d64_ln_back_tan(const double* __restrict__ gamma, const double* y, const double* dy, double* gy,
                                                double* dgy, double* yhat, double* dyh) {
  const double rs = d64_ln_stats(y, yhat);
  double a1 = 0.0, a2 = 0.0;
#pragma unroll
  for (int o = 0; o < D; ++o) a1 += dy[o];
  a1 /= D;
#pragma unroll
  for (int o = 0; o < D; ++o) a2 = fma(yhat[o], dy[o] - a1, a2);
  a2 /= D;
#pragma unroll
  for (int o = 0; o < D; ++o) dyh[o] = rs * ((dy[o] - a1) - yhat[o] * a2);
  const double drs = -rs * rs * a2;   // d (var + eps)^(-1/2) = -rs^3 / 2 * dvar, dvar = 2 mean(yhat dy) / rs
  double m1 = 0.0, m2 = 0.0, dm1 = 0.0, dm2 = 0.0;
#pragma unroll
  for (int o = 0; o < D; ++o) {
    gy[o] *= gamma[o];
    dgy[o] *= gamma[o];
    m1 += gy[o];
    m2 = fma(gy[o], yhat[o], m2);
    dm1 += dgy[o];
    dm2 = fma(dgy[o], yhat[o], fma(gy[o], dyh[o], dm2));
  }
  m1 /= D;
  m2 /= D;
  dm1 /= D;
  dm2 /= D;
#pragma unroll
  for (int o = 0; o < D; ++o) {
    const double r = gy[o] - m1 - yhat[o] * m2;
    const double dr = dgy[o] - dm1 - dyh[o] * m2 - yhat[o] * dm2;
    gy[o] = rs * r;
    dgy[o] = fma(drs, r, rs * dr);
  }
}

// pg_edges with its tangent: per edge position two sub-rounds, dA (x) B then A (x) dB, in the row layout of pg_edges.  c, dc: the
// lane's rows of C and dC (global; read only when act).
__device__ __forceinline__ void jr_edges(const double* __restrict__ Wp, bool act, const double* x, const double* dx,
                                         const double* __restrict__ cg, const double* __restrict__ dcg, const double* __restrict__ h,
                                         const double* __restrict__ t, int32_t beg, int32_t end, const int32_t* __restrict__ nbr,
                                         const double* __restrict__ attr, double* buf, double* row, double* pt, int base) {
  using L = W64<2>;
  double c[D], dc[D], q[D], dq[D], a1[2] = {0.0, 0.0}, a2[1] = {0.0};
#pragma unroll
  for (int k = 0; k < D; ++k) {
    c[k] = act ? cg[k] : 0.0;
    dc[k] = act ? dcg[k] : 0.0;
  }
  d64_w2t(Wp, c, q);
  d64_w2t(Wp, dc, dq);
  for (int32_t j = 0;; ++j) {
    const bool on = act && beg + j < end;
    if (!__syncthreads_or(on)) break;   // also the barrier behind the previous round's reads
    double xj[D], dxj[D], a[3], s[D], ds[D];
    if (on) {
      const int32_t i = beg + j;
      const int64_t u = nbr[i];
      d64_row(h, u, xj);
      d64_row(t, u, dxj);
#pragma unroll
      for (int k = 0; k < 3; ++k) a[k] = attr[3 * (int64_t)i + k];
      d64_pre(Wp, x, xj, a, s);
#pragma unroll
      for (int o = 0; o < D; ++o) {
        const double* w = Wp + L::PHI_W1 + o * L::EIN;
        double r = 0.0;
#pragma unroll
        for (int k = 0; k < D; ++k) r = fma(w[k], dx[k], r);
#pragma unroll
        for (int k = 0; k < D; ++k) r = fma(w[D + k], dxj[k], r);
        ds[o] = s[o] > 0.0 ? r : 0.0;
      }
      // d qm (x) [x_i, x_j, a, 1]; dc (x) [relu(s), 1]
#pragma unroll
      for (int k = 0; k < D; ++k) {
        row[k] = s[k] > 0.0 ? dq[k] : 0.0;
        row[10 + k] = x[k];
        row[20 + k] = xj[k];
        row[34 + k] = dc[k];
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
  pg_put<2>(pt, base + L::PHI_W1, base + L::PHI_B1, D, L::EIN + 1, a1);
  pg_put<1>(pt, base + L::PHI_W2, base + L::PHI_B2, D, D + 1, a2);
}

// One layer at (h, t, w, dw): dloc (N, D), C and dC (N, CW) and the chunk's partial row of the parameter part.  dw NULL: zero.
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
      al = 1.0 / (1.0 + exp(-al));
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
  jr_edges(W + lofs, upd, x, dx, cg, dcg, h, t, cb, ce, csc_nbr, csc_attr, buf, row, pt, L::layer(0));
  jr_edges(W + lofs + L::PHI_SZ, upd, x, dx, cg + D, dcg + D, h, t, rb, re, csr_nbr, csr_attr, buf, row, pt, L::layer(0) + L::PHI_SZ);
  if (MIXED) jr_edges(W + nofs, neu, x, dx, cg + 2 * D, dcg + 2 * D, h, t, rb, re, csr_nbr, csr_attr, buf, row, pt, L::layer(1));
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
  const unsigned g = (unsigned)cdiv(p->N, 256);
  const int cw = p->mixed ? 3 * D : 2 * D;
  // both edge lists three times (the forward with its tangent, the x_i side, the rounds: neighbour id, 3 attributes, the neighbour's
  // row and -- twice -- its tangent row), per node h, t, w, dw, dloc, C and dC written and read again, flag, pointers and problem
  // data; the partial rows
  PROF_BYTES(2 * p->Ep * (3 * (4 + 24) + 40 * D) + p->N * (8 * (5 * D + 4 * cw) + 8 * (p->mixed ? 5 : 2) + 17) + pg_part_doubles(f) * 8);
  if (p->mixed) {
    using L = W64<3>;
    LAUNCH("k_f64_jr", st,
           (k_f64_jr<3, true, 1><<<(unsigned)nch, PG_ROWS, 0, st>>>(p->N, W, L::layer(l), L::layer(nl), apply_ln, F64_EDGES(f), h, t,
                                                                    prb, nrm, w, dw, C, dloc, dC, part)));
    pg_reduce(part, nch, L::total(1, true), L::SHARED, L::LAYER, L::layer(l), L::layer(nl), grad, st);
    // the Neumann rows: per node flag and pointers, the partial rows once more; the edge reads of the few Neumann rows are not
    // counted (the host does not know how many there are)
    PROF_BYTES(p->N * 17 + pg_part_doubles(f) * 8);
    LAUNCH("k_f64_jr_neumann", st,
           (k_f64_jr<3, true, 2><<<(unsigned)nch, PG_ROWS, 0, st>>>(p->N, W, L::layer(l), L::layer(nl), apply_ln, F64_EDGES(f), h, t,
                                                                    prb, nrm, w, dw, C, dloc, dC, part)));
    pg_reduce(part, nch, L::total(1, true), L::SHARED, L::LAYER, L::layer(l), L::layer(nl), grad, st);
  } else {
    using L = W64<2>;
    LAUNCH("k_f64_jr", st,
           (k_f64_jr<2, false, 0><<<(unsigned)nch, PG_ROWS, 0, st>>>(p->N, W, L::layer(l), L::layer(nl), apply_ln, F64_EDGES(f), h, t, prb,
                                                                  nrm, w, dw, C, dloc, dC, part)));
    pg_reduce(part, nch, L::total(1, false), L::SHARED, L::LAYER, L::layer(l), L::layer(nl), grad, st);
  }
  // pass B on (dloc, dC), masks at h: as in vjp_launch
  PROF_BYTES(2 * p->Ep * (4 + 1 + 24 + 16 * D) + p->N * (8 * 3 * D + 8));
  if (p->mixed) {
    using L = W64<3>;
    LAUNCH("k_f64_vjp_edge", st,
           (k_f64_vjp_edge<true><<<g, 256, 0, st>>>(p->N, W, L::layer(l), L::layer(nl), F64_EDGES(f), h, dloc, dC, nullptr, out,
                                                    nullptr)));
  } else {
    using L = W64<2>;
    LAUNCH("k_f64_vjp_edge", st,
           (k_f64_vjp_edge<false><<<g, 256, 0, st>>>(p->N, W, L::layer(l), L::layer(nl), F64_EDGES(f), h, dloc, dC, nullptr, out,
                                                     nullptr)));
  }
}

// d_dinit (may be NULL) = d psi / d h_initial: the Dirichlet rows of the tangents of the cotangents on the states h_1 .. h_{L-1} of a
// multi-layer dirichlet block (those rows are copies of h_initial, and J_f is evaluated at them); zeros for every other block, whose
// Jacobian does not depend on h_initial.
// ARG_CHECK under the name of the entry point that was called
#define JR_CHECK(cond, msg)                       \
  do {                                            \
    if (!(cond)) {                                \
      psignn_set_error("%s: %s", who, msg);       \
      return PSIGNN_EINVAL;                       \
    }                                             \
  } while (0)
static int vjp_backward_impl(const char* who, psignn_f64_t* f, const double* W, int nl, const double* h, const double* h0,
                             const double* prb, const double* nrm, const double* v, const double* gbar, double* d_grad, double* d_dh,
                             double* d_jtv, double* d_dinit, double* work, int64_t work_doubles, void* stream) {
  JR_CHECK(f && W && h && h0 && prb && v && gbar && d_grad && d_dh, "NULL argument");
  JR_CHECK(nl >= 1 && nl <= 64, "n_layers out of range");
  JR_CHECK(!f->p->mixed || nrm, "mixed plan needs unit normals");
  JR_CHECK(d_dh != h && d_dh != v && d_dh != gbar, "d_dh must not alias h, v or gbar");
  JR_CHECK(d_jtv != h && d_jtv != v && d_jtv != gbar && d_jtv != d_dh, "d_jtv must not alias h, v, gbar or d_dh");
  JR_CHECK(!d_dinit || (d_dinit != h && d_dinit != v && d_dinit != gbar && d_dinit != d_dh && d_dinit != d_jtv),
            "d_dinit must not alias h, v, gbar, d_dh or d_jtv");
  const int rc = work_check(who, psignn_f64_vjp_backward_workspace_doubles(f, nl), work, work_doubles);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipMemsetAsync(d_grad, 0, sizeof(double) * psignn_f64_weights_size(f->p->mixed, nl), st));
  if (f->p->N == 0) return PSIGNN_OK;
  const int64_t row = f->p->N * D;
  const int cw = f->p->mixed ? 3 : 2;
  double *loc = work, *C = work + row, *dloc = C + cw * row, *dC = dloc + row, *rest = dC + cw * row;
  if (!f64_chain(f, nl)) {   // mixed: only the last layer's iteration reaches the output, the earlier layers' sections stay zero
    if (d_dinit) HIP_TRY(hipMemsetAsync(d_dinit, 0, sizeof(double) * row, st));
    jr_launch(f, W, nl, nl - 1, 1, h, gbar, prb, nrm, v, nullptr, C, dloc, dC, rest, d_grad, d_dh, st);
    if (d_jtv) vjp_launch(f, W, nl, nl - 1, 1, h, prb, nrm, v, loc, C, nullptr, d_jtv, nullptr, st);
  } else {
    // the states h_1 .. h_{L-1} at h with their tangents along gbar, then the chain backwards: layer l at (h_l, t_l, w_{l+1}, dw_{l+1})
    double *states = rest, *tans = states + (nl - 1) * row, *wpp = tans + (nl - 1) * row, *dwpp = wpp + 2 * row, *part = dwpp + 2 * row;
    const double *ch = h, *ct = gbar;
    for (int l = 0; l + 1 < nl; ++l) {
      jvp_launch(f, W, nl, l, 0, ch, ct, h0, prb, nullptr, states + l * row, tans + l * row, nullptr, st);
      ch = states + l * row;
      ct = tans + l * row;
    }
    const double *cw_ = v, *cdw = nullptr;
    for (int l = nl - 1; l >= 0; --l) {
      const double* hl = l == 0 ? h : states + (l - 1) * row;
      const double* tl = l == 0 ? gbar : tans + (l - 1) * row;
      double* ddst = l == 0 ? d_dh : dwpp + (l & 1) * row;
      double* dst = l == 0 ? d_jtv : wpp + (l & 1) * row;
      jr_launch(f, W, nl, l, l == nl - 1, hl, tl, prb, nrm, cw_, cdw, C, dloc, dC, part, d_grad, ddst, st);
      if (d_dinit && l > 0) {   // ddst: the tangent of the cotangent on h_l, whose Dirichlet rows are h_initial's
        PROF_BYTES(f->p->N * (1 + 16 * D));
        LAUNCH("k_f64_pg_init", st,
               (k_f64_pg_init<<<(unsigned)cdiv(row, 256), 256, 0, st>>>(f->p->N, f->p->flags, ddst, l != nl - 1, d_dinit)));
      }
      if (dst) vjp_launch(f, W, nl, l, l == nl - 1, hl, prb, nrm, cw_, loc, C, nullptr, dst, nullptr, st);
      cw_ = dst;
      cdw = ddst;
    }
  }
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
