// The node block of f_theta in float64 (gfx950), stated once: what takes a row's [h | Phi_to | Phi_from | prb] (Neumann rows:
// [h | Phi_neumann | prb | normal]) through the gate, the update MLP and LayerNorm, forwards, with a tangent, and backwards.
// Included by fgnn_f64.hip and fgnn_f64_deriv.hip and nothing else; the weight layout W64 is f64_common.h's.
//
// The conventions every float64 kernel takes from here:
//   * a Neumann row is REPLACED by update_neumann(...) (mixed/psignn/model.py:236,241); the gate and the residual act on update rows only;
//   * LayerNorm(10), eps 1e-5, biased variance, affine (model.py:293);
//   * ReLU': 1 where the pre-activation is > 0 (torch's threshold_backward); the mask is a constant of every tangent;
//   * per edge the whole message MLP of the reference, first layer on the concatenated 23 inputs, messages summed per node in the
//     plan's canonical order; every sum is one fma chain in a fixed order, so the same call gives the same bits.
// Every piece is a __forceinline__ template: TAN = false carries no tangent code (its d* arguments may be NULL); NEU picks the
// Neumann-row form or the update-row form, so a kernel that meets both kinds of row calls one form per branch.
// Taken by k_f64_jvp_layer (below), k_f64_vjp_node and k_f64_pgrad.  k_f64_jr (fgnn_f64_deriv.hip) takes the per-edge pieces and
// LayerNorm from here and keeps its own statement of the node with a tangent (see the note at that kernel), so the reverse here
// carries no tangent.
#pragma once
#include "f64_common.h"
#include <math.h>

// ---------------------------------------------------------------------------------------------
// per edge
// ---------------------------------------------------------------------------------------------
// s = W1 [x_i; x_j; a] + b1, the pre-activations of one message
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
// their tangent along (dx_i, dx_j) under the ReLU mask: t = 1[s > 0] * (W1_i dx_i + W1_j dx_j)
__device__ __forceinline__ void d64_pre_tan(const double* __restrict__ Wp, const double* s, const double* dxi, const double* dxj,
                                            double* t) {
  using L = W64<2>;
#pragma unroll
  for (int o = 0; o < D; ++o) {
    const double* w = Wp + L::PHI_W1 + o * L::EIN;
    double r = 0.0;
#pragma unroll
    for (int k = 0; k < D; ++k) r = fma(w[k], dxi[k], r);
#pragma unroll
    for (int k = 0; k < D; ++k) r = fma(w[D + k], dxj[k], r);
    t[o] = s[o] > 0.0 ? r : 0.0;
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

// Sum of the messages MLP([x_i | x_j | a]) = W2 relu(W1 [x_i; x_j; a] + b1) + b2 of one Phi module over one edge list of node n, and
// (TAN) of their tangents along (dx, v): d message = W2 (1[s > 0] * (W1_i dx + W1_j v_u)).
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
      d64_pre_tan(Wp, s, dx, dxj, t);
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

// ---------------------------------------------------------------------------------------------
// LayerNorm
// ---------------------------------------------------------------------------------------------
// statistics of y; yhat = (y - mu) * rs
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
// tangent of yhat along dy: dyh = rs (dyc - yhat mean(yhat dyc)), dyc = dy - mean(dy); returns mean(yhat dyc).  dyh may be dy.
__device__ __forceinline__ double d64_ln_tan(double rs, const double* yhat, const double* dy, double* dyh) {
  double m1 = 0.0, m2 = 0.0;
#pragma unroll
  for (int o = 0; o < D; ++o) m1 += dy[o];
  m1 /= D;
#pragma unroll
  for (int o = 0; o < D; ++o) m2 = fma(yhat[o], dy[o] - m1, m2);
  m2 /= D;
#pragma unroll
  for (int o = 0; o < D; ++o) dyh[o] = rs * ((dy[o] - m1) - yhat[o] * m2);
  return m2;
}
// forwards: y <- yhat * gamma + beta, dy <- d yhat * gamma
template <bool TAN>
__device__ __forceinline__ void d64_ln_fwd(const double* __restrict__ W, double* y, double* dy) {
  using L = W64<2>;   // the shared section has the same head in both families
  double yhat[D];
  const double rs = d64_ln_stats(y, yhat);
  if (TAN) {
    d64_ln_tan(rs, yhat, dy, dy);
#pragma unroll
    for (int o = 0; o < D; ++o) dy[o] = dy[o] * W[L::LN_G + o];
  }
#pragma unroll
  for (int o = 0; o < D; ++o) y[o] = yhat[o] * W[L::LN_G + o] + W[L::LN_B + o];
}
// gy, the cotangent of LayerNorm's output at y, back through it: gy <- rs (g - mean(g) - yhat mean(g yhat)), g = gamma * gy.
// yhat: the normalised row (a factor of laynorm.weight's gradient).
__device__ __forceinline__ void d64_ln_back(const double* __restrict__ gamma, const double* y, double* gy, double* yhat) {
  double m1 = 0.0, m2 = 0.0;
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

// the gate: sigmoid of alpha's pre-activation
__device__ __forceinline__ double d64_sigmoid(double a) { return 1.0 / (1.0 + exp(-a)); }

// ---------------------------------------------------------------------------------------------
// The node, forwards.  From the row x = h[n] (dx: its tangent; the neighbours' rows and tangents from h, v):
//   cat (dcat)   the MLP's input [h | Phi_to | Phi_from | prb] or [h | Phi_neumann | prb | normal] (the 3 D / 2 D entries with a tangent)
//   al (dal)     the gate sigmoid(alpha(cat)) of an update row; 1 (0) on a Neumann row
//   mask         bit o: hidden pre-activation o is > 0;   rp (drp): relu(pre) and its tangent
//   sv (dsv)     the MLP's output;   y (dy): x + al * sv, or sv alone on a Neumann row -- the layer's value before LayerNorm
// lofs / nofs: the layer's weight block and phi_neumann's.
// ---------------------------------------------------------------------------------------------
template <int P, bool TAN, bool NEU>
__device__ __forceinline__ void d64_node_fwd(const double* W, int lofs, int nofs, int64_t n, const double* x, const double* dx,
                                             const double* h, const double* v, const int32_t* csr_ptr, const int32_t* csr_nbr,
                                             const double* csr_attr, const int32_t* csc_ptr, const int32_t* csc_nbr,
                                             const double* csc_attr, const double* prb, const double* nrm, double* cat, double* dcat,
                                             double& al, double& dal, unsigned& mask, double* rp, double* drp, double* sv, double* dsv,
                                             double* y, double* dy) {
  using L = W64<P>;
#pragma unroll
  for (int k = 0; k < D; ++k) {
    cat[k] = x[k];
    if (TAN) dcat[k] = dx[k];
  }
  al = 1.0, dal = 0.0;
  if (NEU) {   // Phi_neumann has Phi_from's flow: summed at the row index over the out-edges
    d64_phi<TAN>(W + nofs, x, dx, h, v, csr_ptr[n], csr_ptr[n + 1], csr_nbr, csr_attr, cat + D, TAN ? dcat + D : nullptr);
#pragma unroll
    for (int k = 0; k < P; ++k) cat[2 * D + k] = prb[n * P + k];
    cat[2 * D + P] = nrm[2 * n];
    cat[2 * D + P + 1] = nrm[2 * n + 1];
  } else {
    d64_phi<TAN>(W + lofs, x, dx, h, v, csc_ptr[n], csc_ptr[n + 1], csc_nbr, csc_attr, cat + D, TAN ? dcat + D : nullptr);   // Phi_to: in-edges, summed at the column index
    d64_phi<TAN>(W + lofs + L::PHI_SZ, x, dx, h, v, csr_ptr[n], csr_ptr[n + 1], csr_nbr, csr_attr, cat + 2 * D,
                 TAN ? dcat + 2 * D : nullptr);   // Phi_from: out-edges, summed at the row index
#pragma unroll
    for (int k = 0; k < P; ++k) cat[3 * D + k] = prb[n * P + k];
    al = W[L::AL_B];
#pragma unroll
    for (int k = 0; k < L::CAT; ++k) al = fma(W[L::AL_W + k], cat[k], al);
    al = d64_sigmoid(al);
    if (TAN) {
#pragma unroll
      for (int k = 0; k < 3 * D; ++k) dal = fma(W[L::AL_W + k], dcat[k], dal);
      dal *= al * (1.0 - al);
    }
  }
  const double* Wm = NEU ? W + nofs + L::PHI_SZ : W + lofs + 2 * L::PHI_SZ;   // W1 | b1 | W2 | b2 of the row's MLP
  constexpr int ncat = NEU ? L::NCAT : L::CAT, nd = NEU ? 2 * D : 3 * D;   // its inputs, and those of them that carry a tangent
  constexpr int ob1 = NEU ? L::NEU_B1 : L::UPD_B1, ow2 = NEU ? L::NEU_W2 : L::UPD_W2, ob2 = NEU ? L::NEU_B2 : L::UPD_B2;
  mask = 0;
  // (the loops run to the wider bound under a guard, as the kernels wrote them)
#pragma unroll
  for (int o = 0; o < D; ++o) {
    double s = Wm[ob1 + o], r = 0.0;
#pragma unroll
    for (int k = 0; k < L::CAT; ++k)
      if (k < ncat) s = fma(Wm[o * ncat + k], cat[k], s);
    if (TAN) {
#pragma unroll
      for (int k = 0; k < 3 * D; ++k)
        if (k < nd) r = fma(Wm[o * ncat + k], dcat[k], r);
    }
    if (s > 0.0) mask |= 1u << o;
    rp[o] = fmax(s, 0.0);
    if (TAN) drp[o] = s > 0.0 ? r : 0.0;
  }
#pragma unroll
  for (int o = 0; o < D; ++o) {
    double s = Wm[ob2 + o], r = 0.0;
#pragma unroll
    for (int k = 0; k < D; ++k) {
      s = fma(Wm[ow2 + o * D + k], rp[k], s);
      if (TAN) r = fma(Wm[ow2 + o * D + k], drp[k], r);
    }
    sv[o] = s;
    y[o] = NEU ? s : x[o] + al * s;
    if (TAN) {
      dsv[o] = r;
      dy[o] = NEU ? r : dx[o] + dal * s + al * r;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// The node, backwards, in two steps: d64_node_back_q gives gal, g and q, d64_node_back_c from them c and gx.  From gy, the cotangent
// of y (LayerNorm already behind it), and the forward's record:
//   gal   the cotangent of the gate's pre-activation, (gy . sv) al (1 - al); 0 on a Neumann row
//   g     al * gy, the cotangent of the MLP's output;   q = mask * W2^T g, that of the hidden pre-activations
//   c     the cotangents of the message sums: {c_to, c_from} of an update row at c[0 .. 2 D), c_neu of a Neumann row at
//         c[2 D .. 3 D); the caller has zeroed the rest
//   gx    (NULL: not wanted) what reaches x through the MLP's first layer, the gate and the residual
// ---------------------------------------------------------------------------------------------
template <int P, bool NEU>
__device__ __forceinline__ void d64_node_back_q(const double* W, int lofs, int nofs, unsigned mask, double al, const double* sv,
                                                const double* gy, double& gal, double* g, double* q) {
  using L = W64<P>;
  const double* Wm = NEU ? W + nofs + L::PHI_SZ : W + lofs + 2 * L::PHI_SZ;
  constexpr int ow2 = NEU ? L::NEU_W2 : L::UPD_W2;
  gal = 0.0;
  if (!NEU) {   // y = x + al * s
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
    q[k] = (mask >> k) & 1u ? s : 0.0;
  }
}
template <int P, bool NEU>
__device__ __forceinline__ void d64_node_back_c(const double* W, int lofs, int nofs, double gal, const double* q, const double* gy,
                                                double* c, double* gx) {
  using L = W64<P>;
  const double* Wm = NEU ? W + nofs + L::PHI_SZ : W + lofs + 2 * L::PHI_SZ;
  if (NEU) {   // the row is replaced: no residual, no gate
#pragma unroll
    for (int k = 0; k < D; ++k) {
      double s = 0.0, u = 0.0;
#pragma unroll
      for (int o = 0; o < D; ++o) {
        s = fma(Wm[o * L::NCAT + D + k], q[o], s);
        if (gx) u = fma(Wm[o * L::NCAT + k], q[o], u);
      }
      c[2 * D + k] = s;
      if (gx) gx[k] = u;
    }
  } else {
#pragma unroll
    for (int k = 0; k < 3 * D; ++k) {
      double s = W[L::AL_W + k] * gal;
#pragma unroll
      for (int o = 0; o < D; ++o) s = fma(Wm[o * L::CAT + k], q[o], s);
      if (k >= D)
        c[k - D] = s;
      else if (gx)
        gx[k] = gy[k] + s;
    }
  }
}
// gx += the x_i side of the row's own messages, from the cotangents c of its message sums (or, for their tangent, dc)
template <int P, bool NEU>
__device__ __forceinline__ void d64_node_back_xi(const double* W, int lofs, int nofs, const double* x,
                                                 const double* h, int32_t rb, int32_t re, int32_t cb, int32_t ce,
                                                 const int32_t* csr_nbr, const double* csr_attr,
                                                 const int32_t* csc_nbr, const double* csc_attr,
                                                 const double* c, double* gx) {
  using L = W64<P>;
  double q[D];
  if (NEU) {
    d64_w2t(W + nofs, c + 2 * D, q);
    d64_phi_vjp_xi(W + nofs, x, h, rb, re, csr_nbr, csr_attr, q, gx);
  } else {
    d64_w2t(W + lofs, c, q);
    d64_phi_vjp_xi(W + lofs, x, h, cb, ce, csc_nbr, csc_attr, q, gx);
    d64_w2t(W + lofs + L::PHI_SZ, c + D, q);
    d64_phi_vjp_xi(W + lofs + L::PHI_SZ, x, h, rb, re, csr_nbr, csr_attr, q, gx);
  }
}

// ---------------------------------------------------------------------------------------------
// One layer, one node per lane: out_h (may be NULL) the layer's value, out_v (TAN) its tangent along v.  TAN = false is the plain
// layer: f itself (launched as k_f64_layer) and the states of a multi-layer chain (k_f64_state_layer).  done: the flag of a solver
// (NULL: none) -- a launch queued past the solver's last iteration returns at once.
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
  if (fl & FLAG_DIRICHLET) {   // Dirichlet rows <- h_initial rows, last of all (model.py:298; mixed/psignn/model.py:243): tangent 0
#pragma unroll
    for (int o = 0; o < D; ++o) {
      if (out_h) out_h[n * D + o] = h0[n * D + o];
      if (TAN) out_v[n * D + o] = 0.0;
    }
    return;
  }
  double x[D], dx[D], y[D], dy[D], cat[L::CAT], dcat[3 * D], rp[D], drp[D], sv[D], dsv[D], al, dal;
  unsigned mask;
  d64_row(h, n, x);
  if (TAN) d64_row(v, n, dx);
  if (MIXED && (fl & FLAG_NEUMANN))
    d64_node_fwd<P, TAN, true>(W, lofs, nofs, n, x, dx, h, v, csr_ptr, csr_nbr, csr_attr, csc_ptr, csc_nbr, csc_attr, prb, nrm, cat, dcat,
                         al, dal, mask, rp, drp, sv, dsv, y, dy);
  else
    d64_node_fwd<P, TAN, false>(W, lofs, nofs, n, x, dx, h, v, csr_ptr, csr_nbr, csr_attr, csc_ptr, csc_nbr, csc_attr, prb, nrm, cat, dcat,
                         al, dal, mask, rp, drp, sv, dsv, y, dy);
  if (apply_ln) d64_ln_fwd<TAN>(W, y, dy);
#pragma unroll
  for (int o = 0; o < D; ++o) {
    if (out_h) out_h[n * D + o] = y[o];
    if (TAN) out_v[n * D + o] = dy[o];
  }
}
