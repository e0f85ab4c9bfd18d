// Backward passes built on global-gather kernels with an INJECTED cotangent (gfx950; caller's numbering, no atomics):
//   * the backward of the vector-Jacobian product of f_theta (the Jacobian regulariser's double backward) -- below;
//   * the backward of one DS-GPS update and of one DSS update (back-propagation through the baselines' unrolled updates) --
//     at the end of the file.
// All three push a node-level cotangent on c = [h, Phi_to(h), Phi_from(h)(, Phi_neumann(h))] through the same edge-level
// pair k_jr_edge_local / k_jr_edge_remote and leave parameter-gradient records for the MFMA reduction of fgnn_pgrad.hip.
//
// ---- Backward of the vector-Jacobian product of f_theta (both families, single layer)
//
// The reference's Jacobian regulariser  jac_loss = |v^T J_f(H*)|^2 / (N d)  (jac_loss_estimate, dirichlet/psignn/model.py:
// 416-435, one Gaussian probe v) is built with autograd.grad(..., create_graph=True) and enters the training loss with
// weight ``jac_weight`` (training_class.py:156-159; the reference's launch scripts train with jac_weight = 1.0,
// dirichlet/psignn/launch_local.sh:24).  loss.backward() then differentiates the VJP itself ("double backward").
// With g = J^T v and gbar = d loss / d g held constant that derivative is the gradient of the scalar
//     phi(theta, h) = gbar . (J(h, theta)^T v) = v^T J(h, theta) gbar
// i.e. reverse mode through the JVP of f along gbar.  f = LayerNorm(h + alpha(c) * upd(c)) with c = [h, mp_to, mp_fr, prb]:
// the two Phi aggregations are piecewise linear in h (ReLU masks are constants for autograd), so second-order terms exist
// only in the node-level part (sigmoid gate, the product alpha * upd, LayerNorm).  Four steps, no atomics:
//   1. k_jr_tangent (node n): forward aggregations mp = W2 S + deg b2 and their tangents t = W2 S',
//        S' = sum_e 1[z_e > 0] (W1i gbar_n + W1j gbar_u)   (edge-level JVP with the masks of h).
//   2. k_jr_node (node n): forward, tangent (dc = [gbar_n, t_to, t_fr, 0]) and reverse sweep of
//        psi_n = v_n . dN(c_n; dc_n): adjoints cbar = d psi / d c and chat = d psi / d dc (the ordinary VJP factors), and
//        the node-level factors of the parameter gradients.  Every weight M enters as M a (primal) and M da (tangent), so
//        its gradient is  abar_out (x) a + dabar_out (x) da:  two records per node in the layout of the parameter-VJP
//        (fgnn_tile_vjp.hip groups) -- R1 with the primal right factors, R2 with the tangent ones.
//   3. k_jr_edge_local / k_jr_edge_remote: the edge-level backward of fgnn_vjp.hip with the cotangent injected at c:
//        run on R1 (cbar: gradients through S(theta_e), and d phi / d h) and on R2 (chat: the bilinear term
//        chat^T (dE/d theta_e) gbar, whose right factors are gbar and S' and which has no bias / edge-feature part).
//   4. the MFMA outer-product reduction of fgnn_pgrad.hip over the 2 N records.
// Dirichlet rows of f are constants: no node-level terms, they only act as neighbours.
// Mixed family: a Neumann row is update_neumann([h, Phi_neumann(h), prb, normal]) before LayerNorm (mixed/psignn/model.py:
// 236,241) -- piecewise linear up to LayerNorm, so its only second-order term is LayerNorm's; its factors go to the
// record groups 20..29 of the mixed parameter-VJP (fgnn_vjp.hip).
#include "jr_node.h"
#include "workspace.h"

template <bool MIXED>
struct JrDims {
  static constexpr int NP = MIXED ? 3 : 2;      // Phi modules: to, from [, neumann]
  static constexpr int PJ = 2 * NP * D;         // P row: NP primal projections, then NP tangent ones
  static constexpr int NB = MIXED ? 6 : 4;      // B row: Pt, Pf, dS_to, dS_fr [, Pn, dS_n]
};
static_assert(JrDims<true>::PJ == 6 * ws::W && JrDims<false>::PJ == 4 * ws::W && JrDims<true>::NB == 6 && JrDims<false>::NB == 4,
              "ws::jr_scratch / ws::JrWork");


// neighbour-side projections of h (primal) and gbar (tangent): P[n] = { W1j_m h_n : m } { W1j_m gbar_n : m }
template <int P, bool MIXED>
__global__ __launch_bounds__(256) void k_jr_project(int64_t N, const float* __restrict__ W, const float* __restrict__ a,
                                                    const float* __restrict__ b, float* __restrict__ Pb) {
  using L = WLayout<P>;
  using J = JrDims<MIXED>;
  int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  float x[D], t[D];
#pragma unroll 1
  for (int f = 0; f < 2; ++f) {
    load10((f ? b : a) + n * D, x);
    float* dst = Pb + n * J::PJ + f * J::NP * D;
    PHASE();
    matvec10<D, false>(W + L::layer(0) + L::L_TO + L::PHI_W1, L::EIN, D, x, t);
    store10(dst, t);
    PHASE();
    matvec10<D, false>(W + L::layer(0) + L::L_FROM + L::PHI_W1, L::EIN, D, x, t);
    store10(dst + D, t);
    if (MIXED) {
      PHASE();
      matvec10<D, false>(W + L::phi_neu(1) + L::PHI_W1, L::EIN, D, x, t);
      store10(dst + 2 * D, t);
    }
  }
}

// one Phi module at node n: S = sum_e relu(z_e), T = sum_e 1[z_e > 0] (dPi + dPj[u]);  mp = W2 S + deg b2, t = W2 T
template <int PJ>
__device__ __forceinline__ void jr_phi_tangent(const float* __restrict__ Wm, const float* x, const float* gx,
                                               const int32_t* __restrict__ nbr, const float* __restrict__ attr, int32_t eb,
                                               int32_t ee, const float* __restrict__ Pb, int poff, int toff, float* S,
                                               float* T, float* mp, float* tt) {
  using L = WLayout<2>;  // Phi blocks have the same layout in both families
  float Pi[D], dPi[D], z[D], pj[D], dj[D];
#pragma unroll
  for (int o = 0; o < D; ++o) {
    Pi[o] = Wm[L::PHI_B1 + o];
    S[o] = T[o] = 0.f;
  }
  PHASE();
  matvec10<D, true>(Wm + L::PHI_W1, L::EIN, 0, x, Pi);
  PHASE();
  matvec10<D, false>(Wm + L::PHI_W1, L::EIN, 0, gx, dPi);
  PHASE();
  for (int32_t i = eb; i < ee; ++i) {
    const float* Pu = Pb + (int64_t)nbr[i] * PJ;
    load10(Pu + poff, pj);
    load10(Pu + toff, dj);
    edge_z(Wm + L::PHI_W1, Pi, pj, attr[3 * (int64_t)i], attr[3 * (int64_t)i + 1], attr[3 * (int64_t)i + 2], z);
#pragma unroll
    for (int o = 0; o < D; ++o) {
      S[o] += fmaxf(z[o], 0.f);
      T[o] += z[o] > 0.f ? dPi[o] + dj[o] : 0.f;
    }
  }
#pragma unroll
  for (int o = 0; o < D; ++o) mp[o] = (float)(ee - eb) * Wm[L::PHI_B2 + o];
  PHASE();
  matvec10<D, true>(Wm + L::PHI_W2, D, 0, S, mp);
  PHASE();
  matvec10<D, false>(Wm + L::PHI_W2, D, 0, T, tt);
}

// step 1: cb[n] = { mp_to, mp_fr, t_to, t_fr } (Neumann row: { mp_n, -, t_n, - });  rec1 groups 3, 4 (21) = (S | deg);
// rec2 groups 3, 4 (21) = (S' | 0)
template <int P, bool MIXED>
__global__ __launch_bounds__(256) void k_jr_tangent(int64_t N, const float* __restrict__ W,
                                                    const int32_t* __restrict__ csr_ptr, const int32_t* __restrict__ csr_nbr,
                                                    const float* __restrict__ csr_attr, const int32_t* __restrict__ csc_ptr,
                                                    const int32_t* __restrict__ csc_nbr, const float* __restrict__ csc_attr,
                                                    const uint8_t* __restrict__ flags, const float* __restrict__ h,
                                                    const float* __restrict__ gb, const float* __restrict__ Pb,
                                                    float* __restrict__ cb, float* __restrict__ rec1,
                                                    float* __restrict__ rec2) {
  using L = WLayout<P>;
  using J = JrDims<MIXED>;
  int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  const uint8_t fl = flags[n];
  if (fl & FLAG_DIRICHLET) return;  // k_jr_node clears the row's records
  float x[D], gx[D], S[D], T[D], mp[D], tt[D];
  load10(h + n * D, x);
  load10(gb + n * D, gx);
  const int32_t ib = csc_ptr[n], ie = csc_ptr[n + 1], ob = csr_ptr[n], oe = csr_ptr[n + 1];
  float* c = cb + n * 4 * D;
  float* r1 = rec1 + n * ws::rec_f(MIXED);
  float* r2 = rec2 + n * ws::rec_f(MIXED);
  if (MIXED && (fl & FLAG_NEUMANN)) {  // Phi_neumann is of the Phi_from type: out-edges
    jr_phi_tangent<J::PJ>(W + L::phi_neu(1), x, gx, csr_nbr, csr_attr, ob, oe, Pb, 2 * D, J::NP * D + 2 * D, S, T, mp, tt);
    store10(c, mp);
    store10(c + 2 * D, tt);
    rec_group(r1 + 21 * 16, S, D, (float)(oe - ob));
    rec_group(r2 + 21 * 16, T, D);
    return;
  }
  jr_phi_tangent<J::PJ>(W + L::layer(0) + L::L_TO, x, gx, csc_nbr, csc_attr, ib, ie, Pb, 0, J::NP * D, S, T, mp, tt);
  store10(c, mp);
  store10(c + 2 * D, tt);
  rec_group(r1 + 3 * 16, S, D, (float)(ie - ib));
  rec_group(r2 + 3 * 16, T, D);
  PHASE();
  jr_phi_tangent<J::PJ>(W + L::layer(0) + L::L_FROM, x, gx, csr_nbr, csr_attr, ob, oe, Pb, D, J::NP * D + D, S, T, mp, tt);
  store10(c + D, mp);
  store10(c + 3 * D, tt);
  rec_group(r1 + 4 * 16, S, D, (float)(oe - ob));
  rec_group(r2 + 4 * 16, T, D);
}

// step 2: node-level second order.  dir1[n] = d psi / d c_h (the direct part of d phi / d h).
// LN = false: an intermediate layer of a multi-layer dirichlet block (no LayerNorm: psi = w . dy, so ybar = 0, dybar = w and
// no laynorm factors); launched as "k_jr_node_noln"
template <int P, bool MIXED, bool LN = true>
__global__ __launch_bounds__(256) void k_jr_node(int64_t N, const float* __restrict__ W, const uint8_t* __restrict__ flags,
                                                 const float* __restrict__ h, const float* __restrict__ prb,
                                                 const float* __restrict__ nrm, const float* __restrict__ v,
                                                 const float* __restrict__ gb, const float* __restrict__ cb,
                                                 float* __restrict__ dir1, float* __restrict__ rec1,
                                                 float* __restrict__ rec2) {
  using L = WLayout<P>;
  constexpr int NG = ws::rec_f(MIXED) / 16;
  int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  const float* Wu = W + L::layer(0) + L::L_UPD;
  const float* Wa = W + L::AL_W;
  float* r1 = rec1 + n * ws::rec_f(MIXED);
  float* r2 = rec2 + n * ws::rec_f(MIXED);
  const uint8_t fl = flags[n];
  float x[D], gx[D];
  load10(h + n * D, x);
  load10(gb + n * D, gx);
  rec_group(r1, x, D, 1.f);   // right factor of the W1 products, also for rows that only act as neighbours
  rec_group(r2, gx, D);
  if (fl & FLAG_DIRICHLET) {
    float zero[D];
#pragma unroll
    for (int o = 0; o < D; ++o) zero[o] = 0.f;
    store10(dir1 + n * D, zero);
    rec_zero(r1, 1, 12);
    rec_zero(r1, 14, MIXED ? 27 : NG);
    rec_zero(r2, 1, 12);
    rec_zero(r2, 14, MIXED ? 27 : NG);
    if (MIXED) {
      rec_zero(r1, 28, NG);
      rec_zero(r2, 28, NG);
    }
    return;
  }
  float w[D], pq[P + 2];
  load10(v + n * D, w);
#pragma unroll
  for (int k = 0; k < P; ++k) pq[k] = prb[n * P + k];
  pq[P] = pq[P + 1] = 0.f;

  if (MIXED && (fl & FLAG_NEUMANN)) return;  // k_jr_node_neumann

  // ---------------------------------------------------------------------------------------------- interior row
  float mpt[D], mpf[D], tt[D], tf[D];
  load10(cb + n * 4 * D, mpt);
  load10(cb + n * 4 * D + D, mpf);
  load10(cb + n * 4 * D + 2 * D, tt);
  load10(cb + n * 4 * D + 3 * D, tf);
  // forward, tangent and reverse sweep of the row: the statements shared with the tile kernel (jr_node.h)
#define JR_NODE_BODY
#define JR_NODE_DIR(c) store10(dir1 + n * D, c)
#include "jr_node.h"
#undef JR_NODE_DIR
#undef JR_NODE_BODY
  if (MIXED) {  // the Neumann branch's factors (27 comes from the remote pass)
    rec_zero(r1, 20, 27);
    rec_zero(r1, 28, NG);
    rec_zero(r2, 20, 27);
    rec_zero(r2, 28, NG);
  }
}

// step 2, Neumann rows of the mixed family (a kernel of its own: together with the interior branch the compiler would keep
// > 1 000 spilled SGPRs alive)
// (Its forward is its own statement of the unfolded Neumann update: the tangent and the record writes stand between its statements.)
template <int P>
__global__ __launch_bounds__(256) void k_jr_node_neumann(int64_t N, const float* __restrict__ W,
                                                         const uint8_t* __restrict__ flags, const float* __restrict__ h,
                                                         const float* __restrict__ prb, const float* __restrict__ nrm,
                                                         const float* __restrict__ v, const float* __restrict__ gb,
                                                         const float* __restrict__ cb, float* __restrict__ dir1,
                                                         float* __restrict__ rec1, float* __restrict__ rec2) {
  using L = WLayout<P>;
  int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  const uint8_t fl = flags[n];
  if ((fl & FLAG_DIRICHLET) || !(fl & FLAG_NEUMANN)) return;
  float* r1 = rec1 + n * ws::rec_f(true);
  float* r2 = rec2 + n * ws::rec_f(true);
  float x[D], gx[D], w[D], pq[P + 2];
  load10(h + n * D, x);
  load10(gb + n * D, gx);
  load10(v + n * D, w);
  rec_group(r1, x, D, 1.f);
  rec_group(r2, gx, D);
#pragma unroll
  for (int k = 0; k < P; ++k) pq[k] = prb[n * P + k];
  // ------------------------------------------------ Neumann row: y = N2 relu(N1 [h, mp_n, prb, normal] + nb1) + nb2
  const float* Un = W + L::upd_neu(1);
  float mpn[D], tn[D];
  load10(cb + n * 4 * D, mpn);
  load10(cb + n * 4 * D + 2 * D, tn);
  pq[P] = nrm[n * 2];
  pq[P + 1] = nrm[n * 2 + 1];
  float q[D], dq[D], hid[D], dhid[D], y[D], dy[D];
#pragma unroll
  for (int o = 0; o < D; ++o) q[o] = Un[L::NEU_B1 + o];
  PHASE();
  matvec10<D, true>(Un + L::NEU_W1, L::NEU_CAT, 0, x, q);
  PHASE();
  matvec10<D, true>(Un + L::NEU_W1, L::NEU_CAT, D, mpn, q);
  PHASE();
  matvec10<P + 2, true>(Un + L::NEU_W1, L::NEU_CAT, 2 * D, pq, q);
  PHASE();
  matvec10<D, false>(Un + L::NEU_W1, L::NEU_CAT, 0, gx, dq);
  PHASE();
  matvec10<D, true>(Un + L::NEU_W1, L::NEU_CAT, D, tn, dq);
  rec_group(r1 + 20 * 16, mpn, D, pq[0], pq[1], pq[2], pq[3], pq[P + 1]);
  rec_group(r2 + 20 * 16, tn, D);
#pragma unroll
  for (int o = 0; o < D; ++o) {
    hid[o] = fmaxf(q[o], 0.f);
    dhid[o] = q[o] > 0.f ? dq[o] : 0.f;
    y[o] = Un[L::NEU_B2 + o];
  }
  PHASE();
  matvec10<D, true>(Un + L::NEU_W2, D, 0, hid, y);
  PHASE();
  matvec10<D, false>(Un + L::NEU_W2, D, 0, dhid, dy);
  rec_group(r1 + 22 * 16, hid, D, 1.f);
  rec_group(r2 + 22 * 16, dhid, D);
  float ybar[D], dybar[D], gln[D];
  PHASE();
  jr_layernorm(W + L::LN_G, w, y, dy, ybar, dybar, gln);
  rec_group(r1 + 14 * 16, gln, D);
  rec_group(r1 + 26 * 16, ybar, D);
  rec_group(r2 + 26 * 16, dybar, D);
  float qb[D], dqb[D], ch[D], cm[D];
  PHASE();
  matvecT<D, false>(Un + L::NEU_W2, D, 0, ybar, qb);
  PHASE();
  matvecT<D, false>(Un + L::NEU_W2, D, 0, dybar, dqb);
#pragma unroll
  for (int o = 0; o < D; ++o) {
    qb[o] = q[o] > 0.f ? qb[o] : 0.f;
    dqb[o] = q[o] > 0.f ? dqb[o] : 0.f;
  }
  rec_group(r1 + 23 * 16, qb, D);
  rec_group(r2 + 23 * 16, dqb, D);
  PHASE();
  matvecT<D, false>(Un + L::NEU_W1, L::NEU_CAT, 0, qb, ch);
  PHASE();
  matvecT<D, false>(Un + L::NEU_W1, L::NEU_CAT, D, qb, cm);
  store10(dir1 + n * D, ch);
  rec_group(r1 + 25 * 16, cm, D);
  PHASE();
  matvecT<D, false>(Un + L::NEU_W1, L::NEU_CAT, D, dqb, cm);
  rec_group(r2 + 25 * 16, cm, D);
  // the interior branch's factors; 12 / 13 / 27 come from the remote pass, 21 / 24 / 28.. from the edge passes
  rec_zero(r1, 1, 12);
  rec_zero(r1, 15, 20);
  rec_zero(r2, 1, 12);
  rec_zero(r2, 14, 20);
}

// masked cotangent sums of one Phi module over node n's own edges: gs = sum_e 1[z_e > 0] dS, and (ATTR) its
// edge-feature moments mom[o * 3 + c] = sum_e 1[z_e[o] > 0] dS[o] a_e[c]
template <int PJ, bool ATTR>
__device__ __forceinline__ void jr_phi_backward(const float* __restrict__ Wm, const float* Pi, const float* dS,
                                                const int32_t* __restrict__ nbr, const float* __restrict__ attr, int32_t eb,
                                                int32_t ee, const float* __restrict__ Pb, int poff, float* gs, float* mom) {
  using L = WLayout<2>;
  float z[D], pj[D];
#pragma unroll
  for (int o = 0; o < D; ++o) gs[o] = 0.f;
  PHASE();
  for (int32_t i = eb; i < ee; ++i) {
    const float a0 = attr[3 * (int64_t)i], a1 = attr[3 * (int64_t)i + 1], a2 = attr[3 * (int64_t)i + 2];
    load10(Pb + (int64_t)nbr[i] * PJ + poff, pj);
    edge_z(Wm + L::PHI_W1, Pi, pj, a0, a1, a2, z);
#pragma unroll
    for (int o = 0; o < D; ++o) {
      const float m = z[o] > 0.f ? dS[o] : 0.f;
      gs[o] += m;
      if (ATTR) {
        mom[o * 3] = fmaf(m, a0, mom[o * 3]);
        mom[o * 3 + 1] = fmaf(m, a1, mom[o * 3 + 1]);
        mom[o * 3 + 2] = fmaf(m, a2, mom[o * 3 + 2]);
      }
    }
  }
}

// step 3a: edge-level backward of the cotangent held in groups 9 / 10 (25) of `rec` (masks of h).  TAN: the record's right
// factors are tangents (no bias, no edge-feature part) and no d / d h is produced.
template <int P, bool MIXED, bool TAN>
__global__ __launch_bounds__(256) void k_jr_edge_local(int64_t N, const float* __restrict__ W,
                                                       const int32_t* __restrict__ csr_ptr, const int32_t* __restrict__ csr_nbr,
                                                       const float* __restrict__ csr_attr, const int32_t* __restrict__ csc_ptr,
                                                       const int32_t* __restrict__ csc_nbr, const float* __restrict__ csc_attr,
                                                       const uint8_t* __restrict__ flags, const float* __restrict__ h,
                                                       const float* __restrict__ Pb, const float* __restrict__ dir,
                                                       float* __restrict__ B, float* __restrict__ out,
                                                       float* __restrict__ rec) {
  using L = WLayout<P>;
  using J = JrDims<MIXED>;
  int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  const float* Wto = W + L::layer(0) + L::L_TO;
  const float* Wfr = W + L::layer(0) + L::L_FROM;
  const float* Wn = W + L::phi_neu(1);
  float* Bn = B + n * J::NB * D;
  const uint8_t fl = flags[n];
  float zero[D];
#pragma unroll
  for (int o = 0; o < D; ++o) zero[o] = 0.f;
  if (fl & FLAG_DIRICHLET) {  // sends nothing
#pragma unroll
    for (int k = 0; k < J::NB; ++k) store10(Bn + k * D, zero);
    if (!TAN) store10(out + n * D, zero);
    return;
  }
  float* r = rec + n * ws::rec_f(MIXED);
  const int32_t ib = csc_ptr[n], ie = csc_ptr[n + 1], ob = csr_ptr[n], oe = csr_ptr[n + 1];
  float x[D], g[D];
  load10(h + n * D, x);
  if (!TAN) load10(dir + n * D, g);

  if (MIXED && (fl & FLAG_NEUMANN)) {
    float Pn[D], dmn[D], dSn[D], gn[D], mom[32];
#pragma unroll
    for (int o = 0; o < D; ++o) {
      Pn[o] = Wn[L::PHI_B1 + o];
      dmn[o] = r[25 * 16 + o];
    }
#pragma unroll
    for (int i = 0; i < 32; ++i) mom[i] = 0.f;
    PHASE();
    matvec10<D, true>(Wn + L::PHI_W1, L::EIN, 0, x, Pn);
    PHASE();
    matvecT<D, false>(Wn + L::PHI_W2, D, 0, dmn, dSn);
#pragma unroll
    for (int k = 0; k < 4; ++k) store10(Bn + k * D, zero);
    store10(Bn + 4 * D, Pn);
    store10(Bn + 5 * D, dSn);
    jr_phi_backward<J::PJ, !TAN>(Wn, Pn, dSn, csr_nbr, csr_attr, ob, oe, Pb, 2 * D, gn, mom);
    rec_group(r + 24 * 16, gn, D);
#pragma unroll
    for (int i = 0; i < 8; ++i)
      reinterpret_cast<float4*>(r + 28 * 16)[i] = make_float4(mom[4 * i], mom[4 * i + 1], mom[4 * i + 2], mom[4 * i + 3]);
    if (!TAN) {
      PHASE();
      matvecT<D, true>(Wn + L::PHI_W1, L::EIN, 0, gn, g);
      store10(out + n * D, g);
    }
    return;
  }

  float Pt[D], Pf[D], dmt[D], dmf[D], dSt[D], dSf[D];
#pragma unroll
  for (int o = 0; o < D; ++o) {
    Pt[o] = Wto[L::PHI_B1 + o];
    Pf[o] = Wfr[L::PHI_B1 + o];
    dmt[o] = r[9 * 16 + o];
    dmf[o] = r[10 * 16 + o];
  }
  PHASE();
  matvec10<D, true>(Wto + L::PHI_W1, L::EIN, 0, x, Pt);
  PHASE();
  matvec10<D, true>(Wfr + L::PHI_W1, L::EIN, 0, x, Pf);
  PHASE();
  matvecT<D, false>(Wto + L::PHI_W2, D, 0, dmt, dSt);
  PHASE();
  matvecT<D, false>(Wfr + L::PHI_W2, D, 0, dmf, dSf);
  store10(Bn, Pt);
  store10(Bn + D, Pf);
  store10(Bn + 2 * D, dSt);
  store10(Bn + 3 * D, dSf);
  if (MIXED) {
    store10(Bn + 4 * D, zero);
    store10(Bn + 5 * D, zero);
  }
  float gt[D], gf[D], mom[64];
#pragma unroll
  for (int i = 0; i < 64; ++i) mom[i] = 0.f;
  jr_phi_backward<J::PJ, !TAN>(Wto, Pt, dSt, csc_nbr, csc_attr, ib, ie, Pb, 0, gt, mom);
  jr_phi_backward<J::PJ, !TAN>(Wfr, Pf, dSf, csr_nbr, csr_attr, ob, oe, Pb, D, gf, mom + 30);
  rec_group(r + 7 * 16, gt, D);
  rec_group(r + 8 * 16, gf, D);
  mom[60] = mom[61] = mom[62] = mom[63] = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i)
    reinterpret_cast<float4*>(r + 16 * 16)[i] = make_float4(mom[4 * i], mom[4 * i + 1], mom[4 * i + 2], mom[4 * i + 3]);
  if (!TAN) {
    PHASE();
    matvecT<D, true>(Wto + L::PHI_W1, L::EIN, 0, gt, g);
    PHASE();
    matvecT<D, true>(Wfr + L::PHI_W1, L::EIN, 0, gf, g);
    store10(out + n * D, g);
  }
}

// step 3b: what node u receives as somebody's neighbour (groups 12 / 13 (27), and out += W1j^T acc)
template <int P, bool MIXED, bool TAN>
__global__ __launch_bounds__(256) void k_jr_edge_remote(int64_t N, const float* __restrict__ W,
                                                        const int32_t* __restrict__ csr_ptr, const int32_t* __restrict__ csr_nbr,
                                                        const float* __restrict__ csr_attr, const int32_t* __restrict__ csc_ptr,
                                                        const int32_t* __restrict__ csc_nbr, const float* __restrict__ csc_attr,
                                                        const float* __restrict__ Pb, const float* __restrict__ B,
                                                        float* __restrict__ out, float* __restrict__ rec) {
  using L = WLayout<P>;
  using J = JrDims<MIXED>;
  int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= N) return;
  const float* Wto = W + L::layer(0) + L::L_TO;
  const float* Wfr = W + L::layer(0) + L::L_FROM;
  const float* Wn = W + L::phi_neu(1);
  float pjt[D], pjf[D], pjn[D], at[D], af[D], an[D], z[D];
  load10(Pb + u * J::PJ, pjt);
  load10(Pb + u * J::PJ + D, pjf);
  if (MIXED) load10(Pb + u * J::PJ + 2 * D, pjn);
#pragma unroll
  for (int o = 0; o < D; ++o) at[o] = af[o] = an[o] = 0.f;
  PHASE();
  for (int32_t i = csr_ptr[u]; i < csr_ptr[u + 1]; ++i) {  // u -> n: Phi_to terms of n that read h[u]
    const float* Bn = B + (int64_t)csr_nbr[i] * J::NB * D;
    float pt[D], ds[D];
    load10(Bn, pt);
    load10(Bn + 2 * D, ds);
    edge_z(Wto + L::PHI_W1, pt, pjt, csr_attr[3 * (int64_t)i], csr_attr[3 * (int64_t)i + 1], csr_attr[3 * (int64_t)i + 2], z);
#pragma unroll
    for (int o = 0; o < D; ++o) at[o] += z[o] > 0.f ? ds[o] : 0.f;
  }
  PHASE();
  for (int32_t i = csc_ptr[u]; i < csc_ptr[u + 1]; ++i) {  // n -> u: Phi_from (Phi_neumann) terms of n that read h[u]
    const float* Bn = B + (int64_t)csc_nbr[i] * J::NB * D;
    const float a0 = csc_attr[3 * (int64_t)i], a1 = csc_attr[3 * (int64_t)i + 1], a2 = csc_attr[3 * (int64_t)i + 2];
    float pf[D], ds[D];
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
  float* r = rec + u * ws::rec_f(MIXED);
  rec_group(r + 12 * 16, at, D);
  rec_group(r + 13 * 16, af, D);
  if (MIXED) rec_group(r + 27 * 16, an, D);
  if (!TAN) {
    float g[D];
    load10(out + u * D, g);
    PHASE();
    matvecT<D, true>(Wto + L::PHI_W1, L::EIN, D, at, g);
    PHASE();
    matvecT<D, true>(Wfr + L::PHI_W1, L::EIN, D, af, g);
    if (MIXED) {
      PHASE();
      matvecT<D, true>(Wn + L::PHI_W1, L::EIN, D, an, g);
    }
    store10(out + u * D, g);
  }
}

template <int P, bool MIXED>
static void jr_launch(const psignn_plan* p, const float* W, const float* h, const float* prb, const float* nrm, const float* v,
                      const float* gbar, float* out_h, float* work, float* rec1, float* rec2, hipStream_t st, bool ln = true) {
  const int64_t N = p->N;
  const unsigned grid = (unsigned)cdiv(N, 256);
  const ws::JrScratch sc = ws::jr_scratch(N, MIXED, work);
  float *Pb = sc.P, *cb = sc.cb, *B = sc.B, *dir = sc.dir;
#define JR_CSR p->csr_ptr, p->csr_nbr, p->csr_attr, p->csc_ptr, p->csc_nbr, p->csc_attr
  LAUNCH("k_jr_project", st, (k_jr_project<P, MIXED><<<grid, 256, 0, st>>>(N, W, h, gbar, Pb)));
  LAUNCH("k_jr_tangent", st, (k_jr_tangent<P, MIXED><<<grid, 256, 0, st>>>(N, W, JR_CSR, p->flags, h, gbar, Pb, cb, rec1, rec2)));
  if (ln) {
    LAUNCH("k_jr_node", st, (k_jr_node<P, MIXED><<<grid, 256, 0, st>>>(N, W, p->flags, h, prb, nrm, v, gbar, cb, dir, rec1, rec2)));
  } else if constexpr (!MIXED) {
    // reads h, prb, v, gbar, cb (40 + 8 + 40 + 40 + 160 bytes per node), writes dir and the two node-level record sets
    PROF_BYTES((int64_t)N * (288 + 40 + 2 * ws::rec_f(MIXED) * 4));
    LAUNCH("k_jr_node_noln", st, (k_jr_node<P, false, false><<<grid, 256, 0, st>>>(N, W, p->flags, h, prb, nrm, v, gbar, cb, dir, rec1, rec2)));
  }
  if constexpr (MIXED)
    LAUNCH("k_jr_node_neumann", st, (k_jr_node_neumann<P><<<grid, 256, 0, st>>>(N, W, p->flags, h, prb, nrm, v, gbar, cb, dir, rec1, rec2)));
  LAUNCH("k_jr_edge_local", st, (k_jr_edge_local<P, MIXED, false><<<grid, 256, 0, st>>>(N, W, JR_CSR, p->flags, h, Pb, dir, B, out_h, rec1)));
  LAUNCH("k_jr_edge_remote", st, (k_jr_edge_remote<P, MIXED, false><<<grid, 256, 0, st>>>(N, W, JR_CSR, Pb, B, out_h, rec1)));
  LAUNCH("k_jr_edge_local", st, (k_jr_edge_local<P, MIXED, true><<<grid, 256, 0, st>>>(N, W, JR_CSR, p->flags, h, Pb, dir, B, nullptr, rec2)));
  LAUNCH("k_jr_edge_remote", st, (k_jr_edge_remote<P, MIXED, true><<<grid, 256, 0, st>>>(N, W, JR_CSR, Pb, B, nullptr, rec2)));
#undef JR_CSR
}

// work: ws::jr_scratch (<= N * 170 floats);  rec1, rec2: (N, 320 | 480) each, the two record sets (ws::JrWork);
// out_h: (N, 10) = d phi / d h
// ln = 0: the LayerNorm-off form (an intermediate layer of a multi-layer dirichlet block).  W: a single-layer weight view.
int psignn_jacreg_records(const psignn_plan* p, const float* W, const float* h, const float* prb, const float* nrm,
                          const float* v, const float* gbar, float* out_h, float* work, float* rec1, float* rec2, hipStream_t st,
                          int ln) {
  ARG_CHECK(ln || !p->mixed, "the LayerNorm-off backward of the VJP is a dirichlet-family form");
  if (p->mixed)
    jr_launch<3, true>(p, W, h, prb, nrm, v, gbar, out_h, work, rec1, rec2, st);
  else
    jr_launch<2, false>(p, W, h, prb, nrm, v, gbar, out_h, work, rec1, rec2, st, ln != 0);
  HIP_TRY(hipGetLastError());
  return PSIGNN_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// DS-GPS: backward of one recurrent update (dirichlet/dsgps/model.py:72-89), for back-propagation through the k unrolled
// updates of ModelDSGPS.forward (training the baseline, dirichlet/dsgps/training_class.py).  Same two Phi aggregations as
// f_theta, then  z = sigma(Wz c + bz), r = sigma(Wr c + br), corr = tanh(Wc [r h, mp_to, mp_fr, prb] + bc),
// h' = h + z corr, Dirichlet rows <- H_0.  The node kernel turns the cotangent w on h' into the cotangent on
// c = [h, mp_to, mp_fr] and the gate factors; the edge-level backward is the injected-cotangent pair above.  The Phi
// weights come in the f_theta layout (WLayout<P>: phi_to / phi_from blocks of layer 0; mixed family: also phi_neumann and
// update_neumann -- a Neumann row is replaced by update_neumann([h, Phi_neumann(h), prb, normal]), mixed/dsgps/model.py:79-93),
// the gates as Wg = [Wz (10 x (30+P)) | bz | Wr | br | Wc | bc] (nn.Linear layout).  Record groups (320 floats, reduced with TabG in
// fgnn_pgrad.hip): 0 x|1, 1 mp_to|prb, 2 mp_fr, 3 S_to|deg, 4 S_fr|deg, 5 r h|1, 6 d pre_z, 7 gt, 8 gf, 9 d mp_to,
// 10 d mp_fr, 11 d pre_r, 12 acc_t, 13 acc_f, 14 d pre_c, 16..19 dS (.) attr.
// ---------------------------------------------------------------------------------------------------------------------
template <int P, bool MIXED>
__global__ __launch_bounds__(256) void k_ds_phi(int64_t N, const float* __restrict__ W, const int32_t* __restrict__ csr_ptr,
                                                const int32_t* __restrict__ csr_nbr, const float* __restrict__ csr_attr,
                                                const int32_t* __restrict__ csc_ptr, const int32_t* __restrict__ csc_nbr,
                                                const float* __restrict__ csc_attr, const uint8_t* __restrict__ flags,
                                                const float* __restrict__ h, const float* __restrict__ Pb,
                                                float* __restrict__ cb, float* __restrict__ rec) {
  using L = WLayout<P>;
  using J = JrDims<MIXED>;
  int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  const uint8_t fl = flags[n];
  if (fl & FLAG_DIRICHLET) return;
  float x[D], S[D], T[D], mp[D], tt[D];
  load10(h + n * D, x);
  float* c = cb + n * 4 * D;
  float* r = rec + n * ws::rec_f(MIXED);
  if (MIXED && (fl & FLAG_NEUMANN)) {
    jr_phi_tangent<J::PJ>(W + L::phi_neu(1), x, x, csr_nbr, csr_attr, csr_ptr[n], csr_ptr[n + 1], Pb, 2 * D, J::NP * D + 2 * D, S, T, mp, tt);
    store10(c, mp);
    rec_group(r + 21 * 16, S, D, (float)(csr_ptr[n + 1] - csr_ptr[n]));
    return;
  }
  jr_phi_tangent<J::PJ>(W + L::layer(0) + L::L_TO, x, x, csc_nbr, csc_attr, csc_ptr[n], csc_ptr[n + 1], Pb, 0, J::NP * D, S, T, mp, tt);
  store10(c, mp);
  rec_group(r + 3 * 16, S, D, (float)(csc_ptr[n + 1] - csc_ptr[n]));
  PHASE();
  jr_phi_tangent<J::PJ>(W + L::layer(0) + L::L_FROM, x, x, csr_nbr, csr_attr, csr_ptr[n], csr_ptr[n + 1], Pb, D, J::NP * D + D, S, T, mp, tt);
  store10(c + D, mp);
  rec_group(r + 4 * 16, S, D, (float)(csr_ptr[n + 1] - csr_ptr[n]));
}

// gate pre-activation  out[o] = b[o] + W[o, 0:10] . a + W[o, 10:20] . mt + W[o, 20:30] . mf + W[o, 30:30+P] . pq
template <int P>
__device__ __forceinline__ void ds_gate(const float* __restrict__ Wm, const float* a, const float* mt, const float* mf,
                                        const float* pq, float* out) {
  constexpr int CAT = 3 * D + P;
#pragma unroll
  for (int o = 0; o < D; ++o) out[o] = Wm[D * CAT + o];
  PHASE();
  matvec10<D, true>(Wm, CAT, 0, a, out);
  PHASE();
  matvec10<D, true>(Wm, CAT, D, mt, out);
  PHASE();
  matvec10<D, true>(Wm, CAT, 2 * D, mf, out);
  PHASE();
  matvec10<P, true>(Wm, CAT, 3 * D, pq, out);
}

// Wf: the Phi modules (and, mixed, update_neumann) in the f_theta layout; Wg: the gates
template <int P, bool MIXED>
__global__ __launch_bounds__(256) void k_ds_node_bwd(int64_t N, const float* __restrict__ Wf, const float* __restrict__ Wg,
                                                     const uint8_t* __restrict__ flags, const float* __restrict__ h,
                                                     const float* __restrict__ prb, const float* __restrict__ nrm,
                                                     const float* __restrict__ wv, const float* __restrict__ cb,
                                                     float* __restrict__ dir, float* __restrict__ rec) {
  using L = WLayout<P>;
  constexpr int NG = ws::rec_f(MIXED) / 16;
  constexpr int CAT = 3 * D + P, GSZ = D * CAT + D;
  int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  float* r = rec + n * ws::rec_f(MIXED);
  const uint8_t fl = flags[n];
  float x[D];
  load10(h + n * D, x);
  rec_group(r, x, D, 1.f);
  if (fl & FLAG_DIRICHLET) {  // the row is a copy of H_0: its cotangent goes there (host side), nothing flows through
    float zero[D];
#pragma unroll
    for (int o = 0; o < D; ++o) zero[o] = 0.f;
    store10(dir + n * D, zero);
    rec_zero(r, 1, 12);
    rec_zero(r, 14, MIXED ? 27 : NG);
    if (MIXED) rec_zero(r, 28, NG);
    return;
  }
  float w[D], pq[P + 2];
  load10(wv + n * D, w);
#pragma unroll
  for (int k = 0; k < P; ++k) pq[k] = prb[n * P + k];
  pq[P] = pq[P + 1] = 0.f;
  if (MIXED && (fl & FLAG_NEUMANN)) {  // h' = N2 relu(N1 [h, mp_n, prb, normal] + nb1) + nb2 (the row is replaced)
    const float* Un = Wf + L::upd_neu(1);
    float mpn[D], q[D], hid[D], dq[D], g[D], dm[D];
    load10(cb + n * 4 * D, mpn);
    pq[P] = nrm[n * 2];
    pq[P + 1] = nrm[n * 2 + 1];
#pragma unroll
    for (int o = 0; o < D; ++o) q[o] = Un[L::NEU_B1 + o];
    PHASE();
    matvec10<D, true>(Un + L::NEU_W1, L::NEU_CAT, 0, x, q);
    PHASE();
    matvec10<D, true>(Un + L::NEU_W1, L::NEU_CAT, D, mpn, q);
    PHASE();
    matvec10<P + 2, true>(Un + L::NEU_W1, L::NEU_CAT, 2 * D, pq, q);
#pragma unroll
    for (int o = 0; o < D; ++o) hid[o] = fmaxf(q[o], 0.f);
    PHASE();
    matvecT<D, false>(Un + L::NEU_W2, D, 0, w, dq);
#pragma unroll
    for (int o = 0; o < D; ++o) dq[o] = q[o] > 0.f ? dq[o] : 0.f;
    PHASE();
    matvecT<D, false>(Un + L::NEU_W1, L::NEU_CAT, 0, dq, g);
    PHASE();
    matvecT<D, false>(Un + L::NEU_W1, L::NEU_CAT, D, dq, dm);
    store10(dir + n * D, g);
    rec_zero(r, 1, 12);
    rec_zero(r, 14, 20);
    rec_group(r + 20 * 16, mpn, D, pq[0], pq[1], pq[2], pq[3], pq[P + 1]);
    rec_group(r + 22 * 16, hid, D, 1.f);
    rec_group(r + 23 * 16, dq, D);
    rec_group(r + 25 * 16, dm, D);
    rec_group(r + 26 * 16, w, D);
    return;
  }
  const float* Wz = Wg;
  const float* Wr = Wg + GSZ;
  const float* Wc = Wg + 2 * GSZ;
  float mt[D], mf[D];
  load10(cb + n * 4 * D, mt);
  load10(cb + n * 4 * D + D, mf);
  rec_group(r + 16, mt, D, pq[0], pq[1], P > 2 ? pq[P - 1] : 0.f);
  rec_group(r + 2 * 16, mf, D);
  float z[D], rr[D], rx[D], co[D];
  ds_gate<P>(Wz, x, mt, mf, pq, z);
  PHASE();
  ds_gate<P>(Wr, x, mt, mf, pq, rr);
#pragma unroll
  for (int o = 0; o < D; ++o) {
    z[o] = 1.f / (1.f + expf(-z[o]));
    rr[o] = 1.f / (1.f + expf(-rr[o]));
    rx[o] = rr[o] * x[o];
  }
  PHASE();
  ds_gate<P>(Wc, rx, mt, mf, pq, co);
  rec_group(r + 5 * 16, rx, D, 1.f);
  float dpc[D], dpz[D], dpr[D], dx[D], dmt[D], dmf[D], t[D];
#pragma unroll
  for (int o = 0; o < D; ++o) {
    co[o] = tanhf(co[o]);
    dpc[o] = w[o] * z[o] * (1.f - co[o] * co[o]);
    dpz[o] = w[o] * co[o] * z[o] * (1.f - z[o]);
  }
  PHASE();
  matvecT<D, false>(Wc, CAT, 0, dpc, t);            // cotangent of r h
  PHASE();
  matvecT<D, false>(Wc, CAT, D, dpc, dmt);
  PHASE();
  matvecT<D, false>(Wc, CAT, 2 * D, dpc, dmf);
#pragma unroll
  for (int o = 0; o < D; ++o) {
    dpr[o] = t[o] * x[o] * rr[o] * (1.f - rr[o]);
    dx[o] = fmaf(t[o], rr[o], w[o]);                   // through r h, and the residual path h' = h + ...
  }
  rec_group(r + 14 * 16, dpc, D);
  PHASE();
  matvecT<D, true>(Wz, CAT, 0, dpz, dx);
  PHASE();
  matvecT<D, true>(Wz, CAT, D, dpz, dmt);
  PHASE();
  matvecT<D, true>(Wz, CAT, 2 * D, dpz, dmf);
  PHASE();
  matvecT<D, true>(Wr, CAT, 0, dpr, dx);
  PHASE();
  matvecT<D, true>(Wr, CAT, D, dpr, dmt);
  PHASE();
  matvecT<D, true>(Wr, CAT, 2 * D, dpr, dmf);
  store10(dir + n * D, dx);
  rec_group(r + 6 * 16, dpz, D);
  rec_group(r + 9 * 16, dmt, D);
  rec_group(r + 10 * 16, dmf, D);
  rec_group(r + 11 * 16, dpr, D);
  rec_zero(r, 15, 16);
  if (MIXED) {
    rec_zero(r, 20, 27);
    rec_zero(r, 28, NG);
  }
}

template <int P, bool MIXED>
static void ds_launch(const psignn_plan* p, const float* Wf, const float* Wg, const float* h, const float* prb, const float* nrm,
                      const float* w, float* out_h, float* work, float* rec, hipStream_t st) {
  const int64_t N = p->N;
  const unsigned grid = (unsigned)cdiv(N, 256);
  const ws::JrScratch sc = ws::jr_scratch(N, MIXED, work);
  float *Pb = sc.P, *cb = sc.cb, *B = sc.B, *dir = sc.dir;
#define JR_CSR p->csr_ptr, p->csr_nbr, p->csr_attr, p->csc_ptr, p->csc_nbr, p->csc_attr
  LAUNCH("k_jr_project", st, (k_jr_project<P, MIXED><<<grid, 256, 0, st>>>(N, Wf, h, h, Pb)));
  LAUNCH("k_ds_phi", st, (k_ds_phi<P, MIXED><<<grid, 256, 0, st>>>(N, Wf, JR_CSR, p->flags, h, Pb, cb, rec)));
  LAUNCH("k_ds_node_bwd", st, (k_ds_node_bwd<P, MIXED><<<grid, 256, 0, st>>>(N, Wf, Wg, p->flags, h, prb, nrm, w, cb, dir, rec)));
  LAUNCH("k_jr_edge_local", st, (k_jr_edge_local<P, MIXED, false><<<grid, 256, 0, st>>>(N, Wf, JR_CSR, p->flags, h, Pb, dir, B, out_h, rec)));
  LAUNCH("k_jr_edge_remote", st, (k_jr_edge_remote<P, MIXED, false><<<grid, 256, 0, st>>>(N, Wf, JR_CSR, Pb, B, out_h, rec)));
#undef JR_CSR
}

// work: ws::jr_scratch;  rec: (N, 320 | 480);  out_h: (N, 10) = w^T d step / d h
int psignn_dsgps_step_records(const psignn_plan* p, const float* Wf, const float* Wg, const float* h, const float* prb,
                              const float* nrm, const float* w, float* out_h, float* work, float* rec, hipStream_t st) {
  if (p->mixed)
    ds_launch<3, true>(p, Wf, Wg, h, prb, nrm, w, out_h, work, rec, st);
  else
    ds_launch<2, false>(p, Wf, Wg, h, prb, nrm, w, out_h, work, rec, st);
  HIP_TRY(hipGetLastError());
  return PSIGNN_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// DSS: backward of one update  h' = h + alpha Psi_t([h, Phi_to_t(h), Phi_from_t(h), b'])  (dirichlet/dss/model.py:75-83), for
// back-propagation through the k updates of DeepStatisticalSolver.forward.  Psi_t is a two-layer MLP: the node-level part is
// the f_theta update MLP without gate and LayerNorm, so update t's weights come in the f_theta layout with three node
// inputs (WLayout<3>: phi_to / phi_from with the scalar edge feature in the third attr column, Psi in the update slots) and
// the records reduce with the f_theta table.  No row is constant: the DSS plan has no Dirichlet flags.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_dss_node_bwd(int64_t N, const float* __restrict__ Wf, float alpha,
                                                      const float* __restrict__ h, const float* __restrict__ bp,
                                                      const float* __restrict__ wv, const float* __restrict__ cb,
                                                      float* __restrict__ dir, float* __restrict__ rec) {
  using L = WLayout<3>;
  int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  const float* Wu = Wf + L::layer(0) + L::L_UPD;
  float* r = rec + n * ws::rec_f(false);
  float x[D], mt[D], mf[D], w[D], pq[3];
  load10(h + n * D, x);
  load10(cb + n * 4 * D, mt);
  load10(cb + n * 4 * D + D, mf);
  load10(wv + n * D, w);
#pragma unroll
  for (int k = 0; k < 3; ++k) pq[k] = bp[n * 3 + k];
  rec_group(r, x, D, 1.f);
  rec_group(r + 16, mt, D, pq[0], pq[1], pq[2]);
  rec_group(r + 2 * 16, mf, D);
  float q[D], hid[D], du[D], dq[D], g[D], dmt[D], dmf[D];
#pragma unroll
  for (int o = 0; o < D; ++o) q[o] = Wu[L::UPD_B1 + o];
  PHASE();
  matvec10<D, true>(Wu + L::UPD_W1, L::CAT, 0, x, q);
  PHASE();
  matvec10<D, true>(Wu + L::UPD_W1, L::CAT, D, mt, q);
  PHASE();
  matvec10<D, true>(Wu + L::UPD_W1, L::CAT, 2 * D, mf, q);
  PHASE();
  matvec10<3, true>(Wu + L::UPD_W1, L::CAT, 3 * D, pq, q);
#pragma unroll
  for (int o = 0; o < D; ++o) {
    hid[o] = fmaxf(q[o], 0.f);
    du[o] = alpha * w[o];
    g[o] = w[o];   // residual path h' = h + ...
  }
  PHASE();
  matvecT<D, false>(Wu + L::UPD_W2, D, 0, du, dq);
#pragma unroll
  for (int o = 0; o < D; ++o) dq[o] = q[o] > 0.f ? dq[o] : 0.f;
  PHASE();
  matvecT<D, true>(Wu + L::UPD_W1, L::CAT, 0, dq, g);
  PHASE();
  matvecT<D, false>(Wu + L::UPD_W1, L::CAT, D, dq, dmt);
  PHASE();
  matvecT<D, false>(Wu + L::UPD_W1, L::CAT, 2 * D, dq, dmf);
  store10(dir + n * D, g);
  rec_group(r + 5 * 16, hid, D, 1.f);
  rec_group(r + 6 * 16, dq, D);
  rec_group(r + 9 * 16, dmt, D);
  rec_group(r + 10 * 16, dmf, D);
  rec_group(r + 11 * 16, du, D);
  rec_zero(r, 14, 16);
}

// work: ws::jr_scratch (dirichlet shape);  rec: (N, 320);  out_h: (N, 10) = w^T d step / d h
int psignn_dss_step_records(const psignn_plan* p, const float* Wf, float alpha, const float* h, const float* bp,
                            const float* w, float* out_h, float* work, float* rec, hipStream_t st) {
  const int64_t N = p->N;
  const unsigned grid = (unsigned)cdiv(N, 256);
  const ws::JrScratch sc = ws::jr_scratch(N, false, work);
  float *Pb = sc.P, *cb = sc.cb, *B = sc.B, *dir = sc.dir;
#define JR_CSR p->csr_ptr, p->csr_nbr, p->csr_attr, p->csc_ptr, p->csc_nbr, p->csc_attr
  LAUNCH("k_jr_project", st, (k_jr_project<3, false><<<grid, 256, 0, st>>>(N, Wf, h, h, Pb)));
  LAUNCH("k_ds_phi", st, (k_ds_phi<3, false><<<grid, 256, 0, st>>>(N, Wf, JR_CSR, p->flags, h, Pb, cb, rec)));
  LAUNCH("k_dss_node_bwd", st, (k_dss_node_bwd<<<grid, 256, 0, st>>>(N, Wf, alpha, h, bp, w, cb, dir, rec)));
  LAUNCH("k_jr_edge_local", st, (k_jr_edge_local<3, false, false><<<grid, 256, 0, st>>>(N, Wf, JR_CSR, p->flags, h, Pb, dir, B, out_h, rec)));
  LAUNCH("k_jr_edge_remote", st, (k_jr_edge_remote<3, false, false><<<grid, 256, 0, st>>>(N, Wf, JR_CSR, Pb, B, out_h, rec)));
#undef JR_CSR
  HIP_TRY(hipGetLastError());
  return PSIGNN_OK;
}
