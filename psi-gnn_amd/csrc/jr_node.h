// Node-level second order of the backward of the vector-Jacobian product of f_theta (gfx950), shared by the global-gather kernel
// (gather_backward.hip, k_jr_node) and the tile kernel (fgnn_tile_jr.hip, k_jr_tile_a).  Derivation and record groups: the
// head of gather_backward.hip (step 2).
//
// Included without JR_NODE_BODY: the per-lane helpers.  Included with JR_NODE_BODY defined, INSIDE a kernel: the arithmetic of
// one interior row as a block of statements -- the forward, the tangent (dc = [gx, tt, tf, 0]) and the reverse sweep of
// psi = w . dN(c; dc) at c = [x, mpt, mpf, pq].  A textual block and not a function on purpose: as an inlined function the same
// statements left k_jr_node with other registers and spills (119 / 118 VGPRs, 571 / 573 and 558 / 554 spilled SGPRs), and the
// existing instantiations were to keep their code (profiles/jr_tiled_resource_usage.txt).  It calls the shared helpers of
// fgnn_common.h (matvecT, rec_group, rec_zero) but keeps its own forward: its gate sums x, mp_to and mp_from interleaved per
// index -- another summation order than k_node's or k_vjp_local's gate -- and the tangent and the record writes stand between its
// statements.  So a function form shared with those kernels was not tried again and there are no newer figures than those above:
// the statements differ in substance (other bits), which rules a shared forward out before registers are counted.
//   in scope:  P, LN (template parameters), L = WLayout<P>, W (packed weights), Wu, Wa (update and gate blocks),
//              float x[D], gx[D], w[D], pq[>= P], mpt[D], mpf[D], tt[D], tf[D];  float *r1, *r2 (the row's two records)
//   writes:    the node-level groups 1, 2, 5, 6, 9, 10, 11, 14, 15 of r1 and r2 (0: the kernel; 3, 4, 7, 8, 12, 13, 16..19: the edge
//              level)
//   defines:   float ch[D] = d psi / d c_h, (ct[D], cf[D]) = cbar on (mp_to, mp_fr), (ct2[D], cf2[D]) = chat on their tangents
//   JR_NODE_DIR(ch): what to do with ch once it is complete (the gather kernel stores it)
#ifndef JR_NODE_BODY
#ifndef PSIGNN_JR_NODE_H
#define PSIGNN_JR_NODE_H
#include "fgnn_common.h"

// LayerNorm of y with tangent dy and probe w: psi = sum_o w_o gamma_o dyhat_o.  Returns ybar = d psi / d y,
// dybar = d psi / d dy (the first-order LayerNorm backward of w) and gln = d psi / d gamma.
__device__ __forceinline__ void jr_layernorm(const float* __restrict__ W, const float* w, float* y, const float* dy, float* ybar,
                                             float* dybar, float* gln) {
  // (the statistics are stated inline at every LayerNorm site of the float32 kernels: as a shared function they changed the bits of
  // k_jr_node<2, false, true>, whose subtractions y - mean the compiler then pairs up and no longer contracts with the mean's multiply)
  float mu = 0.f, var = 0.f;
#pragma unroll
  for (int o = 0; o < D; ++o) mu += y[o];
  mu *= (1.f / D);
#pragma unroll
  for (int o = 0; o < D; ++o) {
    const float c = y[o] - mu;
    var = fmaf(c, c, var);
  }
  var *= (1.f / D);
  const float rs = 1.f / sqrtf(var + 1e-5f);
  float p[D], m1 = 0.f, m2 = 0.f, P1 = 0.f, P2 = 0.f;
#pragma unroll
  for (int o = 0; o < D; ++o) {
    y[o] = (y[o] - mu) * rs;  // normalised
    p[o] = w[o] * W[o];       // W = ln_gamma
    m1 += dy[o];
    m2 = fmaf(y[o], dy[o], m2);
    P1 += p[o];
    P2 = fmaf(p[o], y[o], P2);
  }
  m1 *= (1.f / D);
  m2 *= (1.f / D);
  P1 *= (1.f / D);
  P2 *= (1.f / D);
  // dyhat = rs (dy - m1 - yhat m2)
  float psi = 0.f, yhb[D], Y1 = 0.f, Y2 = 0.f;
#pragma unroll
  for (int o = 0; o < D; ++o) {
    const float dyh = rs * (dy[o] - m1 - y[o] * m2);
    gln[o] = w[o] * dyh;
    psi = fmaf(p[o], dyh, psi);
    dybar[o] = rs * (p[o] - P1 - y[o] * P2);
    yhb[o] = -rs * (dy[o] * P2 + p[o] * m2);   // adjoint of yhat
    Y1 += yhb[o];
    Y2 = fmaf(yhb[o], y[o], Y2);
  }
  Y1 *= (1.f / D);
  Y2 *= (1.f / D);
#pragma unroll
  for (int o = 0; o < D; ++o) ybar[o] = rs * (yhb[o] - Y1 - y[o] * Y2) - psi * rs * y[o] * (1.f / D);  // last term: rs itself
}
#endif   // PSIGNN_JR_NODE_H

#else   // JR_NODE_BODY
  float a = W[L::AL_B], da = 0.f;
  PHASE();
#pragma unroll
  for (int k = 0; k < D; ++k) {
    a = fmaf(Wa[k], x[k], a);
    a = fmaf(Wa[D + k], mpt[k], a);
    a = fmaf(Wa[2 * D + k], mpf[k], a);
    da = fmaf(Wa[k], gx[k], da);
    da = fmaf(Wa[D + k], tt[k], da);
    da = fmaf(Wa[2 * D + k], tf[k], da);
  }
#pragma unroll
  for (int k = 0; k < P; ++k) a = fmaf(Wa[3 * D + k], pq[k], a);
  PHASE();
  const float al = 1.f / (1.f + expf(-a));
  const float sp = al * (1.f - al);
  const float dal = sp * da;
  float q[D], dq[D], hid[D], dhid[D], upd[D], dupd[D];
#pragma unroll
  for (int o = 0; o < D; ++o) q[o] = Wu[L::UPD_B1 + o];
  PHASE();
  matvec10<D, true>(Wu + L::UPD_W1, L::CAT, 0, x, q);
  PHASE();
  matvec10<D, true>(Wu + L::UPD_W1, L::CAT, D, mpt, q);
  PHASE();
  matvec10<D, true>(Wu + L::UPD_W1, L::CAT, 2 * D, mpf, q);
  PHASE();
  matvec10<P, true>(Wu + L::UPD_W1, L::CAT, 3 * D, pq, q);
  PHASE();
  matvec10<D, false>(Wu + L::UPD_W1, L::CAT, 0, gx, dq);
  PHASE();
  matvec10<D, true>(Wu + L::UPD_W1, L::CAT, D, tt, dq);
  PHASE();
  matvec10<D, true>(Wu + L::UPD_W1, L::CAT, 2 * D, tf, dq);
  rec_group(r1 + 16, mpt, D, pq[0], pq[1], P > 2 ? pq[P - 1] : 0.f);
  rec_group(r1 + 2 * 16, mpf, D);
  rec_group(r2 + 16, tt, D);
  rec_group(r2 + 2 * 16, tf, D);
#pragma unroll
  for (int o = 0; o < D; ++o) {
    hid[o] = fmaxf(q[o], 0.f);
    dhid[o] = q[o] > 0.f ? dq[o] : 0.f;
    upd[o] = Wu[L::UPD_B2 + o];
  }
  PHASE();
  matvec10<D, true>(Wu + L::UPD_W2, D, 0, hid, upd);
  PHASE();
  matvec10<D, false>(Wu + L::UPD_W2, D, 0, dhid, dupd);
  rec_group(r1 + 5 * 16, hid, D, 1.f);
  rec_group(r2 + 5 * 16, dhid, D);
  float y[D], dy[D], ybar[D], dybar[D], gln[D];
#pragma unroll
  for (int o = 0; o < D; ++o) {
    y[o] = fmaf(al, upd[o], x[o]);
    dy[o] = gx[o] + dal * upd[o] + al * dupd[o];
  }
  PHASE();
  if constexpr (LN) {
    jr_layernorm(W + L::LN_G, w, y, dy, ybar, dybar, gln);
  } else {
#pragma unroll
    for (int o = 0; o < D; ++o) {
      ybar[o] = 0.f;
      dybar[o] = w[o];
      gln[o] = 0.f;
    }
  }
  rec_group(r1 + 14 * 16, gln, D);
  float albar = 0.f, dalbar = 0.f, ub[D], dub[D];
#pragma unroll
  for (int o = 0; o < D; ++o) {
    albar = fmaf(ybar[o], upd[o], albar);
    albar = fmaf(dybar[o], dupd[o], albar);
    dalbar = fmaf(dybar[o], upd[o], dalbar);
    ub[o] = al * ybar[o] + dal * dybar[o];     // adjoint of upd
    dub[o] = al * dybar[o];                    // adjoint of d upd
  }
  const float dabar = dalbar * sp;                       // adjoint of da
  albar = fmaf(dalbar * (1.f - 2.f * al), da, albar);
  const float abar = albar * sp;                         // adjoint of a
  float qb[D], dqb[D];
  PHASE();
  matvecT<D, false>(Wu + L::UPD_W2, D, 0, ub, qb);
  PHASE();
  matvecT<D, false>(Wu + L::UPD_W2, D, 0, dub, dqb);
  rec_group(r1 + 11 * 16, ub, D);
  rec_group(r2 + 11 * 16, dub, D);
#pragma unroll
  for (int o = 0; o < D; ++o) {
    qb[o] = q[o] > 0.f ? qb[o] : 0.f;
    dqb[o] = q[o] > 0.f ? dqb[o] : 0.f;
  }
  // cbar = [ybar, 0, 0] + U1^T qb + w_alpha abar ;  chat = [dybar, 0, 0] + U1^T dqb + w_alpha dabar
  float ch[D], ct[D], cf[D], ct2[D], cf2[D];
  PHASE();
#pragma unroll
  for (int k = 0; k < D; ++k) ch[k] = fmaf(Wa[k], abar, ybar[k]);
  PHASE();
  matvecT<D, true>(Wu + L::UPD_W1, L::CAT, 0, qb, ch);
  PHASE();
  matvecT<D, false>(Wu + L::UPD_W1, L::CAT, D, qb, ct);
  PHASE();
  matvecT<D, false>(Wu + L::UPD_W1, L::CAT, 2 * D, qb, cf);
  PHASE();
#pragma unroll
  for (int k = 0; k < D; ++k) {
    ct[k] = fmaf(Wa[D + k], abar, ct[k]);
    cf[k] = fmaf(Wa[2 * D + k], abar, cf[k]);
  }
  JR_NODE_DIR(ch);
  rec_group(r1 + 6 * 16, qb, D, abar);
  rec_group(r1 + 9 * 16, ct, D);
  rec_group(r1 + 10 * 16, cf, D);
  rec_zero(r1, 15, 16);
  PHASE();
  matvecT<D, false>(Wu + L::UPD_W1, L::CAT, D, dqb, ct2);
  PHASE();
  matvecT<D, false>(Wu + L::UPD_W1, L::CAT, 2 * D, dqb, cf2);
  PHASE();
#pragma unroll
  for (int k = 0; k < D; ++k) {
    ct2[k] = fmaf(Wa[D + k], dabar, ct2[k]);
    cf2[k] = fmaf(Wa[2 * D + k], dabar, cf2[k]);
  }
  rec_group(r2 + 6 * 16, dqb, D, dabar);
  rec_group(r2 + 9 * 16, ct2, D);
  rec_group(r2 + 10 * 16, cf2, D);
  rec_zero(r2, 14, 16);
#endif
