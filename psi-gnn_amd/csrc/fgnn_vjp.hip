// Vector-Jacobian product of f_theta:  out = w^T (d f / d h)  (gfx950), both families (a multi-layer mixed block only
// applies its last layer, mixed/psignn/model.py:221-245; a multi-layer dirichlet block chains this kernel's layers,
// fgnn_layers.hip).
//
// This is what the reference obtains from autograd -- torch.autograd.grad(new_H, H, v) -- inside the implicit
// backward hook (dirichlet/psignn/model.py:210-223: Broyden on y = J^T y + grad), the Hutchinson Jacobian
// regulariser (jac_loss_estimate, model.py:416-435) and the power method (model.py:437-452).  SURVEY §8f-1.
//
// Autograd scatters every edge's cotangent to the neighbour with index_add.  Here the transpose is written as
// two GATHER passes over the plan's CSR/CSC lists, so there are no atomics and the result is reproducible:
//   pass 1 (node n): back through LayerNorm, the gated update MLP and the second Phi layer; keeps
//           B[n] = { Pt[n], Pf[n] (target-side projections incl. bias), dS_to[n], dS_fr[n] [, Pn[n], dS_n[n]] } and
//           writes the node-local part of the result:
//           dy + U1_h^T dq + w_alpha,h * dalpha + W1i_to^T sum_e g_e + W1i_fr^T sum_e g'_e
//           with g_e = dS_to[n] * 1[z_e > 0] over n's in-edges, g'_e likewise over its out-edges;
//   pass 2 (node u): the contributions u receives as somebody's neighbour:
//           for u's out-edges (u -> n), which are in-edges of n:  acc_t += dS_to[n] * 1[Pt[n] + Pjt[u] + At a > 0]
//           for u's in-edges  (n -> u), which are out-edges of n: acc_f += dS_fr[n] * 1[Pf[n] + Pjf[u] + Af a > 0]
//           out[u] += W1j_to^T acc_t + W1j_fr^T acc_f.
// Dirichlet rows of f are constants (their Jacobian rows vanish): they send nothing, but still receive.
// Mixed family: a Neumann row is REPLACED by update_neumann([h, Phi_neumann(h), prb, normal]) before LayerNorm
// (mixed/psignn/model.py:236,241), so its cotangent flows through that branch only (Phi_neumann is of the
// Phi_from type: out-edges of n; pass 2 adds acc_n over u's in-edges).
#include "fgnn_common.h"
#include "internal.h"
#include <string.h>
#include <stdlib.h>

// neighbour-side projections Pj[n] = { W1j_to h_n, W1j_fr h_n [, W1j_neu h_n] }
template <int P, bool MIXED>
__global__ __launch_bounds__(256) void k_vjp_project(int64_t N, const float* __restrict__ W, int lofs, int nofs,
                                                     const float* __restrict__ h, float* __restrict__ Pj) {
  using L = WLayout<P>;
  constexpr int NP = MIXED ? 3 : 2;
  int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  float x[D], t[D];
  load10(h + n * D, x);
  matvec10<D, false>(W + lofs + L::L_TO + L::PHI_W1, L::EIN, D, x, t);
  store10(Pj + n * NP * D, t);
  matvec10<D, false>(W + lofs + L::L_FROM + L::PHI_W1, L::EIN, D, x, t);
  store10(Pj + n * NP * D + D, t);
  if (MIXED) {
    matvec10<D, false>(W + nofs + L::PHI_W1, L::EIN, D, x, t);
    store10(Pj + n * NP * D + 2 * D, t);
  }
}

// Parameter-gradient records (PG mode; reduced by fgnn_pgrad.hip): 16-float groups per node.  Groups 0..19 as written by
// the tiled kernels (fgnn_tile_vjp.hip); the mixed family appends 20: mp_n | prb | normal, 21: S_n | deg_out,
// 22: hid_n | 1, 23: dq_n, 24: gn, 25: d mp_n, 26: dy_n, 27: acc_n (pass 2), 28..29: dS_n (.) attr.
//
// k_vjp_local keeps its own statement of the node block (unfolded gate, update MLP, Neumann update, LayerNorm and its backward).
// The rule for taking a shared piece was: same bits, same occupancy, no more spills.
//   - LayerNorm through a shared function form (statistics + first-order backward), in either row kind: other bits in <3, true, false, true> (the
//     compiler pairs up the subtractions y - mean and no longer contracts them with the mean's multiply).
//   - gate + update through a function form: occupancy changes in <2, false, false, true> and <3, true, false, true>
//     (135 -> 113 / 114 VGPRs, 3 -> 4 waves per SIMD: not a loss, but not the same occupancy, so their timings would have to be
//     made anew), and spilled SGPRs rise in <2, false, true, false> (320 -> 326) and <3, true, false, true> (402 -> 412).
//   - Neumann update alone through a function form: <3, true, false, true> spills 432 SGPRs (402).
// A LayerNorm fix made in ln_fwd_bwd (fgnn_tile_vjp.hip) is made here too.
//
// LN = false: the LayerNorm-off form of an intermediate layer of a multi-layer dirichlet block (launched as "k_vjp_local_noln"):
// dy = w, and the record groups that feed laynorm (14, 15) stay zero
template <int P, bool MIXED, bool PG, bool LN = true>
__global__ __launch_bounds__(256) void k_vjp_local(int64_t N, const float* __restrict__ W, int lofs, int nofs, int unofs,
                                                   const int32_t* __restrict__ csr_ptr, const int32_t* __restrict__ csr_nbr,
                                                   const float* __restrict__ csr_attr, const int32_t* __restrict__ csc_ptr,
                                                   const int32_t* __restrict__ csc_nbr, const float* __restrict__ csc_attr,
                                                   const uint8_t* __restrict__ flags, const float* __restrict__ h,
                                                   const float* __restrict__ prb, const float* __restrict__ nrm,
                                                   const float* __restrict__ wv, const float* __restrict__ Pj,
                                                   float* __restrict__ B, float* __restrict__ out,
                                                   float* __restrict__ rec) {
  using L = WLayout<P>;
  constexpr int REC = ws::rec_f(MIXED);
  constexpr int NP = MIXED ? 3 : 2;   // Pj row = NP * 10 floats
  constexpr int NB = MIXED ? 6 : 4;   // B row  = NB * 10 floats
  int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  const float* Wto = W + lofs + L::L_TO;
  const float* Wfr = W + lofs + L::L_FROM;
  const float* Wn = W + nofs;
  const float* Wu = W + lofs + L::L_UPD;
  const float* Wa = W + L::AL_W;
  const uint8_t fl = flags[n];
  float x[D], Pt[D], Pf[D], Pn[D], zero[D];
  load10(h + n * D, x);
#pragma unroll
  for (int o = 0; o < D; ++o) {
    Pt[o] = Wto[L::PHI_B1 + o];
    Pf[o] = Wfr[L::PHI_B1 + o];
    zero[o] = 0.f;
  }
  PHASE();
  matvec10<D, true>(Wto + L::PHI_W1, L::EIN, 0, x, Pt);
  PHASE();
  matvec10<D, true>(Wfr + L::PHI_W1, L::EIN, 0, x, Pf);
  float* Bn = B + n * NB * D;
  store10(Bn, Pt);
  store10(Bn + D, Pf);
  if (MIXED) {
#pragma unroll
    for (int o = 0; o < D; ++o) Pn[o] = Wn[L::PHI_B1 + o];
    PHASE();
    matvec10<D, true>(Wn + L::PHI_W1, L::EIN, 0, x, Pn);
    store10(Bn + 4 * D, Pn);
  }
  if (fl & FLAG_DIRICHLET) {  // constant row: sends nothing
    store10(Bn + 2 * D, zero);
    store10(Bn + 3 * D, zero);
    if (MIXED) store10(Bn + 5 * D, zero);
    store10(out + n * D, zero);
    if (PG) {  // a constant row still acts as a neighbour: its (x, 1) group feeds the W1j products of pass 2
      float* r = rec + n * REC;
      rec_group(r, x, D, 1.f);
      rec_zero(r, 1, 12);
      rec_zero(r, 14, MIXED ? 27 : 20);
      if (MIXED) rec_zero(r, 28, 30);
    }
    return;
  }
  const int32_t ib = csc_ptr[n], ie = csc_ptr[n + 1], ob = csr_ptr[n], oe = csr_ptr[n + 1];
  float w[D], g[D];
  load10(wv + n * D, w);

  if (MIXED && (fl & FLAG_NEUMANN)) {
    // ------------------------------------------------------------------ Neumann row: y = update_neumann(cat_n)
    const float* Un = W + unofs;
    float S_n[D], z[D], pj[D];
#pragma unroll
    for (int o = 0; o < D; ++o) S_n[o] = 0.f;
    PHASE();
    for (int32_t i = ob; i < oe; ++i) {
      load10(Pj + (int64_t)csr_nbr[i] * NP * D + 2 * D, pj);
      edge_z(Wn + L::PHI_W1, Pn, pj, csr_attr[3 * (int64_t)i], csr_attr[3 * (int64_t)i + 1], csr_attr[3 * (int64_t)i + 2], z);
#pragma unroll
      for (int o = 0; o < D; ++o) S_n[o] += fmaxf(z[o], 0.f);
    }
    float mp_n[D], q[D], hid[D], y[D];
#pragma unroll
    for (int o = 0; o < D; ++o) {
      mp_n[o] = (float)(oe - ob) * Wn[L::PHI_B2 + o];
      q[o] = Un[L::NEU_B1 + o];
    }
    PHASE();
    matvec10<D, true>(Wn + L::PHI_W2, D, 0, S_n, mp_n);
    PHASE();
    matvec10<D, true>(Un + L::NEU_W1, L::NEU_CAT, 0, x, q);
    PHASE();
    matvec10<D, true>(Un + L::NEU_W1, L::NEU_CAT, D, mp_n, q);
    float pq[P + 2];
#pragma unroll
    for (int k = 0; k < P; ++k) pq[k] = prb[n * P + k];
    pq[P] = nrm[n * 2];
    pq[P + 1] = nrm[n * 2 + 1];
    PHASE();
    matvec10<P + 2, true>(Un + L::NEU_W1, L::NEU_CAT, 2 * D, pq, q);
#pragma unroll
    for (int o = 0; o < D; ++o) {
      hid[o] = fmaxf(q[o], 0.f);
      y[o] = Un[L::NEU_B2 + o];
    }
    PHASE();
    matvec10<D, true>(Un + L::NEU_W2, D, 0, hid, y);
    // LayerNorm backward
    float mu = 0.f, var = 0.f;
#pragma unroll
    for (int o = 0; o < D; ++o) mu += y[o];
    mu *= (1.f / D);
#pragma unroll
    for (int o = 0; o < D; ++o) {
      float c = y[o] - mu;
      var = fmaf(c, c, var);
    }
    var *= (1.f / D);
    const float rs = 1.f / sqrtf(var + 1e-5f);
    float dyh[D], dy[D], m1 = 0.f, m2 = 0.f;
#pragma unroll
    for (int o = 0; o < D; ++o) {
      y[o] = (y[o] - mu) * rs;
      dyh[o] = w[o] * W[L::LN_G + o];
      m1 += dyh[o];
      m2 = fmaf(dyh[o], y[o], m2);
    }
    m1 *= (1.f / D);
    m2 *= (1.f / D);
#pragma unroll
    for (int o = 0; o < D; ++o) dy[o] = rs * (dyh[o] - m1 - y[o] * m2);
    float dq[D], dmp_n[D], dS_n[D];
    PHASE();
    matvecT<D, false>(Un + L::NEU_W2, D, 0, dy, dq);
#pragma unroll
    for (int o = 0; o < D; ++o) dq[o] = q[o] > 0.f ? dq[o] : 0.f;
    PHASE();
    matvecT<D, false>(Un + L::NEU_W1, L::NEU_CAT, 0, dq, g);        // no residual path: the row was replaced
    PHASE();
    matvecT<D, false>(Un + L::NEU_W1, L::NEU_CAT, D, dq, dmp_n);
    PHASE();
    matvecT<D, false>(Wn + L::PHI_W2, D, 0, dmp_n, dS_n);
    store10(Bn + 2 * D, zero);
    store10(Bn + 3 * D, zero);
    store10(Bn + 5 * D, dS_n);
    if (PG && MIXED) {  // everything but gn / the attr sums is known here: written before the second edge loop
      float* r = rec + n * REC;
      float t[D];
      rec_group(r, x, D, 1.f);
      rec_zero(r, 1, 12);                                        // the interior branch's factors
#pragma unroll
      for (int o = 0; o < D; ++o) t[o] = w[o] * y[o];
      rec_group(r + 14 * 16, t, D);
      rec_group(r + 15 * 16, w, D);
      rec_zero(r, 16, 20);
      rec_group(r + 20 * 16, mp_n, D, pq[0], pq[1], pq[2], pq[3], pq[4]);
      rec_group(r + 21 * 16, S_n, D, (float)(oe - ob));
      rec_group(r + 22 * 16, hid, D, 1.f);
      rec_group(r + 23 * 16, dq, D);
      rec_group(r + 25 * 16, dmp_n, D);
      rec_group(r + 26 * 16, dy, D);
    }
    float gn[D], dsa[PG ? 32 : 1];
#pragma unroll
    for (int o = 0; o < D; ++o) gn[o] = 0.f;
    if (PG) {
#pragma unroll
      for (int i = 0; i < 32; ++i) dsa[PG ? i : 0] = 0.f;
    }
    PHASE();
    for (int32_t i = ob; i < oe; ++i) {
      const float a0 = csr_attr[3 * (int64_t)i], a1 = csr_attr[3 * (int64_t)i + 1], a2 = csr_attr[3 * (int64_t)i + 2];
      load10(Pj + (int64_t)csr_nbr[i] * NP * D + 2 * D, pj);
      edge_z(Wn + L::PHI_W1, Pn, pj, a0, a1, a2, z);
#pragma unroll
      for (int o = 0; o < D; ++o) {
        const float m = z[o] > 0.f ? dS_n[o] : 0.f;
        gn[o] += m;
        if (PG) {
          dsa[PG ? o * 3 : 0] = fmaf(m, a0, dsa[PG ? o * 3 : 0]);
          dsa[PG ? o * 3 + 1 : 0] = fmaf(m, a1, dsa[PG ? o * 3 + 1 : 0]);
          dsa[PG ? o * 3 + 2 : 0] = fmaf(m, a2, dsa[PG ? o * 3 + 2 : 0]);
        }
      }
    }
    PHASE();
    matvecT<D, true>(Wn + L::PHI_W1, L::EIN, 0, gn, g);
    store10(out + n * D, g);
    if (PG && MIXED) {
      float* r = rec + n * REC;
      rec_group(r + 24 * 16, gn, D);
      dsa[PG ? 30 : 0] = dsa[PG ? 31 : 0] = 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i)
        reinterpret_cast<float4*>(r + 28 * 16)[i] = make_float4(dsa[PG ? 4 * i : 0], dsa[PG ? 4 * i + 1 : 0], dsa[PG ? 4 * i + 2 : 0], dsa[PG ? 4 * i + 3 : 0]);
    }
    return;
  }

  // ---------------------------------------------------------------------- interior row
  float S_to[D], S_fr[D], z[D], pj[D];
#pragma unroll
  for (int o = 0; o < D; ++o) S_to[o] = S_fr[o] = 0.f;
  PHASE();
  for (int32_t i = ib; i < ie; ++i) {
    load10(Pj + (int64_t)csc_nbr[i] * NP * D, pj);
    edge_z(Wto + L::PHI_W1, Pt, pj, csc_attr[3 * (int64_t)i], csc_attr[3 * (int64_t)i + 1], csc_attr[3 * (int64_t)i + 2], z);
#pragma unroll
    for (int o = 0; o < D; ++o) S_to[o] += fmaxf(z[o], 0.f);
  }
  PHASE();
  for (int32_t i = ob; i < oe; ++i) {
    load10(Pj + (int64_t)csr_nbr[i] * NP * D + D, pj);
    edge_z(Wfr + L::PHI_W1, Pf, pj, csr_attr[3 * (int64_t)i], csr_attr[3 * (int64_t)i + 1], csr_attr[3 * (int64_t)i + 2], z);
#pragma unroll
    for (int o = 0; o < D; ++o) S_fr[o] += fmaxf(z[o], 0.f);
  }
  float mp_to[D], mp_fr[D], pq[P];
#pragma unroll
  for (int o = 0; o < D; ++o) {
    mp_to[o] = (float)(ie - ib) * Wto[L::PHI_B2 + o];
    mp_fr[o] = (float)(oe - ob) * Wfr[L::PHI_B2 + o];
  }
  PHASE();
  matvec10<D, true>(Wto + L::PHI_W2, D, 0, S_to, mp_to);
  PHASE();
  matvec10<D, true>(Wfr + L::PHI_W2, D, 0, S_fr, mp_fr);
#pragma unroll
  for (int k = 0; k < P; ++k) pq[k] = prb[n * P + k];
  float al = W[L::AL_B];
#pragma unroll
  for (int k = 0; k < D; ++k) al = fmaf(Wa[k], x[k], al);
#pragma unroll
  for (int k = 0; k < D; ++k) al = fmaf(Wa[D + k], mp_to[k], al);
#pragma unroll
  for (int k = 0; k < D; ++k) al = fmaf(Wa[2 * D + k], mp_fr[k], al);
#pragma unroll
  for (int k = 0; k < P; ++k) al = fmaf(Wa[3 * D + k], pq[k], al);
  al = 1.f / (1.f + expf(-al));
  float q[D], upd[D], y[D], hid[D];
#pragma unroll
  for (int o = 0; o < D; ++o) q[o] = Wu[L::UPD_B1 + o];
  PHASE();
  matvec10<D, true>(Wu + L::UPD_W1, L::CAT, 0, x, q);
  PHASE();
  matvec10<D, true>(Wu + L::UPD_W1, L::CAT, D, mp_to, q);
  PHASE();
  matvec10<D, true>(Wu + L::UPD_W1, L::CAT, 2 * D, mp_fr, q);
  PHASE();
  matvec10<P, true>(Wu + L::UPD_W1, L::CAT, 3 * D, pq, q);
#pragma unroll
  for (int o = 0; o < D; ++o) {
    hid[o] = fmaxf(q[o], 0.f);
    upd[o] = Wu[L::UPD_B2 + o];
  }
  PHASE();
  matvec10<D, true>(Wu + L::UPD_W2, D, 0, hid, upd);
  float mu = 0.f;
#pragma unroll
  for (int o = 0; o < D; ++o) {
    y[o] = fmaf(al, upd[o], x[o]);
    mu += y[o];
  }
  mu *= (1.f / D);
  float var = 0.f;
#pragma unroll
  for (int o = 0; o < D; ++o) {
    float c = y[o] - mu;
    var = fmaf(c, c, var);
  }
  var *= (1.f / D);
  const float rs = 1.f / sqrtf(var + 1e-5f);
  // ---- backward: LayerNorm (LN = false: dy = w; the statistics above are then dead code)
  float dyh[D], dy[D];
  float m1 = 0.f, m2 = 0.f;
#pragma unroll
  for (int o = 0; o < D; ++o) {
    y[o] = (y[o] - mu) * rs;  // normalised
    dyh[o] = w[o] * W[L::LN_G + o];
    m1 += dyh[o];
    m2 = fmaf(dyh[o], y[o], m2);
  }
  m1 *= (1.f / D);
  m2 *= (1.f / D);
  float dal = 0.f, dupd[D];
#pragma unroll
  for (int o = 0; o < D; ++o) {
    dy[o] = LN ? rs * (dyh[o] - m1 - y[o] * m2) : w[o];
    dal = fmaf(dy[o], upd[o], dal);
    dupd[o] = al * dy[o];
    g[o] = dy[o];  // accumulates the node-local result; starts with the residual path y = x + ...
  }
  dal *= al * (1.f - al);
  // ---- update MLP and gate
  float dq[D], dmp_to[D], dmp_fr[D];
  PHASE();
  matvecT<D, false>(Wu + L::UPD_W2, D, 0, dupd, dq);
#pragma unroll
  for (int o = 0; o < D; ++o) dq[o] = q[o] > 0.f ? dq[o] : 0.f;
  PHASE();
  matvecT<D, true>(Wu + L::UPD_W1, L::CAT, 0, dq, g);
  PHASE();
  matvecT<D, false>(Wu + L::UPD_W1, L::CAT, D, dq, dmp_to);
  PHASE();
  matvecT<D, false>(Wu + L::UPD_W1, L::CAT, 2 * D, dq, dmp_fr);
#pragma unroll
  for (int k = 0; k < D; ++k) {
    g[k] = fmaf(Wa[k], dal, g[k]);
    dmp_to[k] = fmaf(Wa[D + k], dal, dmp_to[k]);
    dmp_fr[k] = fmaf(Wa[2 * D + k], dal, dmp_fr[k]);
  }
  // ---- second Phi layer
  float dS_to[D], dS_fr[D];
  PHASE();
  matvecT<D, false>(Wto + L::PHI_W2, D, 0, dmp_to, dS_to);
  PHASE();
  matvecT<D, false>(Wfr + L::PHI_W2, D, 0, dmp_fr, dS_fr);
  store10(Bn + 2 * D, dS_to);
  store10(Bn + 3 * D, dS_fr);
  if (MIXED) store10(Bn + 5 * D, zero);
  // ---- target-side projections: sum of the masked cotangents over the node's own edges
  float gt[D], gf[D], dsa[PG ? 64 : 1];
#pragma unroll
  for (int o = 0; o < D; ++o) gt[o] = gf[o] = 0.f;
  if (PG) {
#pragma unroll
    for (int i = 0; i < 64; ++i) dsa[PG ? i : 0] = 0.f;
  }
  PHASE();
  for (int32_t i = ib; i < ie; ++i) {
    const float a0 = csc_attr[3 * (int64_t)i], a1 = csc_attr[3 * (int64_t)i + 1], a2 = csc_attr[3 * (int64_t)i + 2];
    load10(Pj + (int64_t)csc_nbr[i] * NP * D, pj);
    edge_z(Wto + L::PHI_W1, Pt, pj, a0, a1, a2, z);
#pragma unroll
    for (int o = 0; o < D; ++o) {
      const float m = z[o] > 0.f ? dS_to[o] : 0.f;
      gt[o] += m;
      if (PG) {
        dsa[PG ? o * 3 : 0] = fmaf(m, a0, dsa[PG ? o * 3 : 0]);
        dsa[PG ? o * 3 + 1 : 0] = fmaf(m, a1, dsa[PG ? o * 3 + 1 : 0]);
        dsa[PG ? o * 3 + 2 : 0] = fmaf(m, a2, dsa[PG ? o * 3 + 2 : 0]);
      }
    }
  }
  PHASE();
  for (int32_t i = ob; i < oe; ++i) {
    const float a0 = csr_attr[3 * (int64_t)i], a1 = csr_attr[3 * (int64_t)i + 1], a2 = csr_attr[3 * (int64_t)i + 2];
    load10(Pj + (int64_t)csr_nbr[i] * NP * D + D, pj);
    edge_z(Wfr + L::PHI_W1, Pf, pj, a0, a1, a2, z);
#pragma unroll
    for (int o = 0; o < D; ++o) {
      const float m = z[o] > 0.f ? dS_fr[o] : 0.f;
      gf[o] += m;
      if (PG) {
        dsa[PG ? 30 + o * 3 : 0] = fmaf(m, a0, dsa[PG ? 30 + o * 3 : 0]);
        dsa[PG ? 31 + o * 3 : 0] = fmaf(m, a1, dsa[PG ? 31 + o * 3 : 0]);
        dsa[PG ? 32 + o * 3 : 0] = fmaf(m, a2, dsa[PG ? 32 + o * 3 : 0]);
      }
    }
  }
  PHASE();
  matvecT<D, true>(Wto + L::PHI_W1, L::EIN, 0, gt, g);
  PHASE();
  matvecT<D, true>(Wfr + L::PHI_W1, L::EIN, 0, gf, g);
  store10(out + n * D, g);
  if (PG) {
    float* r = rec + n * REC;
    float t[D];
    rec_group(r, x, D, 1.f);
    rec_group(r + 16, mp_to, D, pq[0], pq[1], P > 2 ? pq[P - 1] : 0.f);
    rec_group(r + 2 * 16, mp_fr, D);
    rec_group(r + 3 * 16, S_to, D, (float)(ie - ib));
    rec_group(r + 4 * 16, S_fr, D, (float)(oe - ob));
    rec_group(r + 5 * 16, hid, D, 1.f);
    rec_group(r + 6 * 16, dq, D, dal);
    rec_group(r + 7 * 16, gt, D);
    rec_group(r + 8 * 16, gf, D);
    rec_group(r + 9 * 16, dmp_to, D);
    rec_group(r + 10 * 16, dmp_fr, D);
    rec_group(r + 11 * 16, dupd, D);
    if constexpr (LN) {
#pragma unroll
      for (int o = 0; o < D; ++o) t[o] = w[o] * y[o];
      rec_group(r + 14 * 16, t, D);
      rec_group(r + 15 * 16, w, D);
    } else {
      rec_zero(r, 14, 16);
    }
    dsa[PG ? 60 : 0] = dsa[PG ? 61 : 0] = dsa[PG ? 62 : 0] = dsa[PG ? 63 : 0] = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i)
      reinterpret_cast<float4*>(r + 16 * 16)[i] = make_float4(dsa[PG ? 4 * i : 0], dsa[PG ? 4 * i + 1 : 0], dsa[PG ? 4 * i + 2 : 0], dsa[PG ? 4 * i + 3 : 0]);
    if (MIXED) {
      rec_zero(r, 20, 27);
      rec_zero(r, 28, 30);
    }
  }
}

template <int P, bool MIXED, bool PG>
__global__ __launch_bounds__(256) void k_vjp_remote(int64_t N, const float* __restrict__ W, int lofs, int nofs,
                                                    const int32_t* __restrict__ csr_ptr, const int32_t* __restrict__ csr_nbr,
                                                    const float* __restrict__ csr_attr, const int32_t* __restrict__ csc_ptr,
                                                    const int32_t* __restrict__ csc_nbr, const float* __restrict__ csc_attr,
                                                    const float* __restrict__ Pj, const float* __restrict__ B,
                                                    float* __restrict__ out, float* __restrict__ rec) {
  using L = WLayout<P>;
  constexpr int NP = MIXED ? 3 : 2;
  constexpr int NB = MIXED ? 6 : 4;
  int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= N) return;
  const float* Wto = W + lofs + L::L_TO;
  const float* Wfr = W + lofs + L::L_FROM;
  const float* Wn = W + nofs;
  float pjt[D], pjf[D], pjn[D], at[D], af[D], an[D], z[D];
  load10(Pj + u * NP * D, pjt);
  load10(Pj + u * NP * D + D, pjf);
  if (MIXED) load10(Pj + u * NP * D + 2 * D, pjn);
#pragma unroll
  for (int o = 0; o < D; ++o) at[o] = af[o] = an[o] = 0.f;
  // u's out-edges (u -> n) are in-edges of n: Phi_to terms of n that read h[u]
  PHASE();
  for (int32_t i = csr_ptr[u]; i < csr_ptr[u + 1]; ++i) {
    const float* Bn = B + (int64_t)csr_nbr[i] * NB * D;
    float pt[D], ds[D];
    load10(Bn, pt);
    load10(Bn + 2 * D, ds);
    edge_z(Wto + L::PHI_W1, pt, pjt, csr_attr[3 * (int64_t)i], csr_attr[3 * (int64_t)i + 1], csr_attr[3 * (int64_t)i + 2], z);
#pragma unroll
    for (int o = 0; o < D; ++o) at[o] += z[o] > 0.f ? ds[o] : 0.f;
  }
  // u's in-edges (n -> u) are out-edges of n: Phi_from (and Phi_neumann) terms of n that read h[u]
  PHASE();
  for (int32_t i = csc_ptr[u]; i < csc_ptr[u + 1]; ++i) {
    const float* Bn = B + (int64_t)csc_nbr[i] * NB * D;
    float pf[D], ds[D];
    const float a0 = csc_attr[3 * (int64_t)i], a1 = csc_attr[3 * (int64_t)i + 1], a2 = csc_attr[3 * (int64_t)i + 2];
    load10(Bn + D, pf);
    load10(Bn + 3 * D, ds);
    edge_z(Wfr + L::PHI_W1, pf, pjf, a0, a1, a2, z);
#pragma unroll
    for (int o = 0; o < D; ++o) af[o] += z[o] > 0.f ? ds[o] : 0.f;
    if (MIXED) {
      load10(Bn + 4 * D, pf);
      load10(Bn + 5 * D, ds);
      edge_z(Wn + L::PHI_W1, pf, pjn, a0, a1, a2, z);
#pragma unroll
      for (int o = 0; o < D; ++o) an[o] += z[o] > 0.f ? ds[o] : 0.f;
    }
  }
  if (PG) {  // neighbour-side cotangent sums: W1j gradients are sum_u acc[u] (x) x[u]
    float* r = rec + u * ws::rec_f(MIXED);
    rec_group(r + 12 * 16, at, D);
    rec_group(r + 13 * 16, af, D);
    if (MIXED) rec_group(r + 27 * 16, an, D);
  }
  float g[D];
  load10(out + u * D, g);
  PHASE();
  matvecT<D, true>(Wto + L::PHI_W1, L::EIN, D, at, g);
  PHASE();
  matvecT<D, true>(Wfr + L::PHI_W1, L::EIN, D, af, g);
  if (MIXED) matvecT<D, true>(Wn + L::PHI_W1, L::EIN, D, an, g);
  store10(out + u * D, g);
}

// layer < 0: the layer a single-layer VJP differentiates (the last one of a mixed block, layer 0 of a dirichlet block);
// layer >= 0 (dirichlet): that layer at its own input state h, LayerNorm on the last layer only (fgnn_layers.hip)
template <int P, bool MIXED, bool PG = false>
static void launch_vjp(const psignn_plan* p, const float* W, int nl, const float* h, const float* prb, const float* nrm,
                       const float* w, float* out, float* work, hipStream_t st, float* rec = nullptr, int layer_ = -1) {
  using L = WLayout<P>;
  const int layer = layer_ >= 0 ? layer_ : (MIXED ? nl - 1 : 0);
  const bool ln = MIXED || layer == nl - 1;
  const int lofs = L::layer(layer), nofs = L::phi_neu(nl), unofs = L::upd_neu(nl);
  const unsigned grid = (unsigned)cdiv(p->N, 256);
  const ws::FVjp v = ws::f_vjp(p->N, MIXED, work, 0);   // Pj (N, 20 | 30) | B (N, 40 | 60)
  float *Pj = v.Pj, *B = v.B;
  LAUNCH("k_vjp_project", st, (k_vjp_project<P, MIXED><<<grid, 256, 0, st>>>(p->N, W, lofs, nofs, h, Pj)));
  if (ln) {
    LAUNCH(PG ? "k_pgrad_local" : "k_vjp_local", st, (k_vjp_local<P, MIXED, PG><<<grid, 256, 0, st>>>(
        p->N, W, lofs, nofs, unofs, p->csr_ptr, p->csr_nbr, p->csr_attr, p->csc_ptr, p->csc_nbr, p->csc_attr, p->flags, h, prb,
        nrm, w, Pj, B, out, rec)));
  } else if constexpr (!MIXED) {
    // reads h, w (40 N each), prb (8 N), flags, CSR + CSC (4 + 4 + 12 bytes per edge each way), Pj per edge (80 bytes);
    // writes B (160 N) and the node-local part (40 N) [+ the records]
    PROF_BYTES(289 * p->N + 120 * (int64_t)p->E + (PG ? (int64_t)p->N * ws::REC_F * 4 : 0));
    LAUNCH(PG ? "k_pgrad_local_noln" : "k_vjp_local_noln", st, (k_vjp_local<2, false, PG, false><<<grid, 256, 0, st>>>(
        p->N, W, lofs, nofs, unofs, p->csr_ptr, p->csr_nbr, p->csr_attr, p->csc_ptr, p->csc_nbr, p->csc_attr, p->flags, h, prb,
        nrm, w, Pj, B, out, rec)));
  }
  LAUNCH(PG ? "k_pgrad_remote" : "k_vjp_remote", st, (k_vjp_remote<P, MIXED, PG><<<grid, 256, 0, st>>>(
      p->N, W, lofs, nofs, p->csr_ptr, p->csr_nbr, p->csr_attr, p->csc_ptr, p->csc_nbr, p->csc_attr, Pj, B, out, rec)));
}

// layer l of a dirichlet block on the gather kernels (caller numbering), LayerNorm on the last layer only; work: N * 60 floats
int psignn_f_gather_vjp_layer(const psignn_plan* p, const float* W, int nl, int l, const float* h, const float* prb,
                              const float* w, float* out, float* work, hipStream_t st) {
  ARG_CHECK(p && !p->mixed && l >= 0 && l < nl, "gather VJP layer: dirichlet plans, 0 <= layer < n_layers");
  launch_vjp<2, false>(p, W, nl, h, prb, nullptr, w, out, work, st, nullptr, l);
  HIP_TRY(hipGetLastError());
  return PSIGNN_OK;
}

// global-gather VJP that also fills the parameter-gradient records (caller's numbering), at layer l (dirichlet: any layer,
// LayerNorm on the last only; mixed: l = nl - 1); work: ws::f_vjp (N * 90 floats at most), rec: N * 320 | 480
int psignn_f_gather_vjp_rec_layer(const psignn_plan* p, const float* W, int nl, int l, const float* h, const float* prb,
                                  const float* nrm, const float* w, float* out, float* work, float* rec, hipStream_t st) {
  ARG_CHECK(l >= 0 && l < nl && (!p->mixed || l == nl - 1), "gather VJP records: bad layer");
  if (p->mixed)
    launch_vjp<3, true, true>(p, W, nl, h, prb, nrm, w, out, work, st, rec, l);
  else
    launch_vjp<2, false, true>(p, W, nl, h, prb, nrm, w, out, work, st, rec, l);
  HIP_TRY(hipGetLastError());
  return PSIGNN_OK;
}

// plan-order VJP: tiled kernels where the plan has tiles, gather kernels otherwise.  Multi-layer dirichlet blocks chain the
// single-layer VJPs (fgnn_layers.hip); their work holds psignn_f_workspace_floats + psignn_f_layers_workspace_floats floats.
extern "C" int psignn_f_vjp_p(const psignn_plan_t* p, const float* W, int nl, const float* h, const float* prb,
                              const float* nrm, const float* w, float* out, float* work, void* stream) {
  ARG_CHECK(p && W && h && prb && w && out && work, "NULL argument");
  ARG_CHECK(out != w && out != h, "out must not alias its inputs");
  if (p->tiled && (p->mixed || nl == 1)) return psignn_f_tile_vjp(p, W, nl, h, prb, nrm, w, out, work, (hipStream_t)stream);
  if (p->tiled) {
    ARG_CHECK(nl >= 1 && nl <= 64, "n_layers out of range");
    return psignn_f_layers_vjp_stateless(p, W, nl, h, prb, w, out, work, work + psignn_f_workspace_floats(p), (hipStream_t)stream);
  }
  return psignn_f_vjp(p, W, nl, h, prb, nrm, w, out, work, stream);
}

extern "C" int psignn_f_vjp(const psignn_plan_t* p, const float* W, int nl, const float* h, const float* prb,
                            const float* nrm, const float* w, float* out, float* work, void* stream) {
  ARG_CHECK(p && W && h && prb && w && out && work, "NULL argument");
  ARG_CHECK(nl >= 1 && nl <= 64, "n_layers out of range");
  ARG_CHECK(!p->mixed || nrm, "mixed plan needs unit normals");
  ARG_CHECK(out != w && out != h, "out must not alias its inputs");
  hipStream_t st = (hipStream_t)stream;
  const bool layers = !p->mixed && nl > 1;   // chain of single-layer VJPs (fgnn_layers.hip); d_work has the layer part too
  float* lw = layers ? work + psignn_f_workspace_floats(p) : nullptr;
  KNOB_INT(mixed_tiled, [] { const char* e = getenv("PSIGNN_MIXED_VJP"); return (int)!(e && strcmp(e, "gather") == 0); }());
  if (p->tiled && (p->mixed ? mixed_tiled : 1)) {
    // caller numbering -> plan order -> tiled kernels -> caller numbering
    ws::Adapter a = ws::f_adapter(p->N, true, work);
    int rc;
    if ((rc = psignn_to_plan(p, h, w, prb, nrm, a, st))) return rc;
    if (layers) rc = psignn_f_layers_vjp_stateless(p, W, nl, a.h, a.prb, a.x, a.out, a.B, lw, st);
    else rc = psignn_f_tile_vjp(p, W, nl, a.h, a.prb, a.nrm, a.x, a.out, a.B, st);
    if (rc) return rc;
    return psignn_from_plan(p, a.out, out, st);
  }
  if (layers) return psignn_f_layers_vjp_stateless(p, W, nl, h, prb, w, out, work, lw, st);
  if (p->mixed)
    launch_vjp<3, true>(p, W, nl, h, prb, nrm, w, out, work, st);
  else
    launch_vjp<2, false>(p, W, nl, h, prb, nrm, w, out, work, st);
  HIP_TRY(hipGetLastError());
  return PSIGNN_OK;
}
