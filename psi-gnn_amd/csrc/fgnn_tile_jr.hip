// Backward of the vector-Jacobian product of f_theta on the tile structures (gfx950; tiled plans of the dirichlet family,
// single-layer block, LayerNorm on; everything in PLAN order, no atomics, fixed summation order).
//
// Gradient of  phi = gbar . (J_f(h)^T v)  w.r.t. the parameters and h -- what loss.backward() leaves behind
// jac_loss_estimate (autograd.grad(f0, z0, v, create_graph=True), dirichlet/psignn/model.py:416-435; jac_weight 1.0 in
// dirichlet/psignn/launch_local.sh:24).  Same mathematics and the same two records per node as the global-gather form
// (gather_backward.hip, steps 1 - 4); only where the operands come from changes:
//   pass A  (k_jr_tile_a)  = k_jr_project + k_jr_tangent + k_jr_node + both k_jr_edge_local launches.
//           stage 1: neighbour-side projections of h (primal) and of gbar (tangent) of tile + halo rows -> LDS, k_jvp_tile's
//                    layout (two arrays of 80-byte rows: values, and behind them tangents);
//           stage 2: one walk per Phi module over the node's pair-merged slots:  S = sum relu(z),  count = sum 1[z > 0], the
//                    edge-feature moments of count, and  sum 1[z > 0] dPj[u];  S' = count (.) dPi + that sum;
//           node level: the statements of k_jr_node (jr_node.h);
//           own edges: dS = W2^T cbar_mp (R1) and dS' = W2^T chat_mp (R2) are per node and meet the masks of h, so the masked
//                    sums over the node's own edges are dS (.) count -- no second sweep (as in k_vjp_tile_a);
//           writes the records of plan node n at positions n (R1) and N + n (R2), the node-local part of d phi / d h, and
//           B[n] = { Pt, dS_to, dS'_to | Pf, dS_fr, dS'_fr }  (60 floats: the half the OUT slots need, then the IN slots' half).
//   pass B  (k_jr_tile_b)  = both k_jr_edge_remote launches: stages one 120-byte half of B[tile + halo] in LDS at a time
//           (768 rows x 240 bytes do not fit) and walks the slots from the neighbour's side, every mask evaluated once for both
//           cotangents:  acc += 1[z > 0] dS (R1: groups 12, 13 and d phi / d h += W1j^T acc),  acc' += 1[z > 0] dS' (R2: groups
//           12, 13 only).
// The records are reduced by k_pgrad_outer<TabF> / k_pgrad_reduce (fgnn_pgrad.hip) over 2 N rows, unchanged.
#include "tile_helpers.h"
#include "jr_node.h"
#include "internal.h"

#define JR_RS 20     // pass A: floats per LDS row [Pj_to | Pj_from]
#define JR_BS 30     // pass B: floats per LDS row [P | dS | dS'] = half a B row

// ---------------------------------------------------------------------------------------------- pass A
// One Phi module over the slots carrying MASK, z = Pi + row[COL..] + AT . a:
//   S[o] += relu(z),  cnt[o] += 1[z > 0],  m[c * 5 + p] += 1[z > 0] a_c,  Tj[o] += 1[z > 0] drow[COL + o]
// (drow = the neighbour's tangent row, doff floats behind its value row).  Returns the number of such slots.
template <int COL, unsigned MASK>
__device__ __forceinline__ float jr_pass_fwd(const uint4* __restrict__ slots, int nslots, const float* __restrict__ lds,
                                             const int doff, const float* __restrict__ AT, const v2f* Pi, v2f* S, v2f* Tj,
                                             v2f* cnt, v2f* m) {
  float deg = 0.f;
  v2f wa[15];
  ld_attr(AT, wa);
  for (SlotWalk<EDGE_PD, MASK> w(slots, nslots); w.more(); w.step())
    if (w.live()) {
      const SlotAttr a = slot_attr(w.slot());
      const float* row = lds + w.row() * JR_RS;
      v2f pj[5], dpj[5], z[5];
      lds_row<COL>(row, pj);
      lds_row<COL>(row + doff, dpj);   // (doff is a multiple of the row stride: same alignment)
      deg += 1.f;
      edge_preact(wa, a, Pi, pj, z);
#pragma unroll
      for (int p = 0; p < 5; ++p) {
        S[p] += __builtin_elementwise_max(z[p], splat(0.f));
        const v2f mk = (v2f){z[p].x > 0.f ? 1.f : 0.f, z[p].y > 0.f ? 1.f : 0.f};
        cnt[p] += mk;
        Tj[p] = __builtin_elementwise_fma(mk, dpj[p], Tj[p]);
        m[p] = __builtin_elementwise_fma(mk, a.a0, m[p]);
        m[5 + p] = __builtin_elementwise_fma(mk, a.a1, m[5 + p]);
        m[10 + p] = __builtin_elementwise_fma(mk, a.a2, m[10 + p]);
      }
    }
  return deg;
}

// lds: 2 x (n_t + n_h) x 80 bytes.  rec: (2 N, 320); B: (N, 60); out: (N, 10)
template <int P>
__global__ __launch_bounds__(256) void k_jr_tile_a(int n_tiles, int chunk, int64_t N, const int32_t* __restrict__ tile_ptr,
                                                   const int32_t* __restrict__ tile_slice, const int32_t* __restrict__ halo,
                                                   const int32_t* __restrict__ halo_cnt, const int32_t* __restrict__ slice_off,
                                                   const uint8_t* __restrict__ slice_deg, const uint4* __restrict__ ell,
                                                   const uint8_t* __restrict__ flags, const float* __restrict__ W, int tofs,
                                                   const float* __restrict__ h, const float* __restrict__ prb,
                                                   const float* __restrict__ wv, const float* __restrict__ gb,
                                                   float* __restrict__ B, float* __restrict__ out, float* __restrict__ rec) {
  using L = WLayout<P>;
  constexpr bool LN = true;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tile = xcd_tile_slot(chunk);
  if (tile >= n_tiles) return;
  const int tid = threadIdx.x;
  const int32_t t0 = tile_ptr[tile];
  const int n_t = tile_ptr[tile + 1] - t0;
  const int n_h = halo_cnt[tile];
  const int32_t* hl = halo + (int64_t)tile * HALO_CAP;
  const float* T = W + tofs;
  const int doff = (n_t + n_h) * JR_RS;   // floats from a node's value row to its tangent row
  // ---- stage 1: neighbour-side projections of the state rows and of the gbar rows of tile + halo -> LDS
  float x[D], gx[D];
  for (int row = tid; row < n_t + n_h; row += TILE_THREADS) {
    const int64_t node = row < n_t ? (int64_t)(t0 + row) : (int64_t)hl[row - n_t];
    float xr[D], vr[D];
    load10(h + node * D, xr);
    load10(gb + node * D, vr);
    if (row == tid) {
#pragma unroll
      for (int o = 0; o < D; ++o) {
        x[o] = xr[o];
        gx[o] = vr[o];
      }
    }
    v2f ta[5], tb[5], da[5], db[5];
#pragma unroll
    for (int p = 0; p < 5; ++p) ta[p] = tb[p] = da[p] = db[p] = splat(0.f);
    PHASE();
    mv2<D>(T + L::T_W1J_TO, xr, ta);
    mv2<D>(T + L::T_W1J_TO, vr, da);
    PHASE();
    mv2<D>(T + L::T_W1J_FR, xr, tb);
    mv2<D>(T + L::T_W1J_FR, vr, db);
    float4* q4 = reinterpret_cast<float4*>(lds + row * JR_RS);
    q4[0] = make_float4(ta[0].x, ta[0].y, ta[1].x, ta[1].y);
    q4[1] = make_float4(ta[2].x, ta[2].y, ta[3].x, ta[3].y);
    q4[2] = make_float4(ta[4].x, ta[4].y, tb[0].x, tb[0].y);
    q4[3] = make_float4(tb[1].x, tb[1].y, tb[2].x, tb[2].y);
    q4[4] = make_float4(tb[3].x, tb[3].y, tb[4].x, tb[4].y);
    float4* qd = reinterpret_cast<float4*>(lds + row * JR_RS + doff);
    qd[0] = make_float4(da[0].x, da[0].y, da[1].x, da[1].y);
    qd[1] = make_float4(da[2].x, da[2].y, da[3].x, da[3].y);
    qd[2] = make_float4(da[4].x, da[4].y, db[0].x, db[0].y);
    qd[3] = make_float4(db[1].x, db[1].y, db[2].x, db[2].y);
    qd[4] = make_float4(db[3].x, db[3].y, db[4].x, db[4].y);
  }
  __syncthreads();
  if (tid >= n_t) return;
  const int64_t n = (int64_t)t0 + tid;
  float* r1 = rec + n * ws::rec_f(false);
  float* r2 = rec + (N + n) * ws::rec_f(false);
  float* Bn = B + n * 2 * JR_BS;
  const uint8_t fl = flags[n];
  rec_group(r1, x, D, 1.f);   // right factor of the W1 products, also for rows that only act as neighbours
  rec_group(r2, gx, D);
  if (fl & FLAG_DIRICHLET) {   // constant row: sends nothing (groups 12, 13: pass B)
    float zero[D];
#pragma unroll
    for (int o = 0; o < D; ++o) zero[o] = 0.f;
    store10(out + n * D, zero);
    for (int i = 0; i < 2 * JR_BS / 2; ++i) reinterpret_cast<float2*>(Bn)[i] = make_float2(0.f, 0.f);
    rec_zero(r1, 1, 12);
    rec_zero(r1, 14, ws::rec_f(false) / 16);
    rec_zero(r2, 1, 12);
    rec_zero(r2, 14, ws::rec_f(false) / 16);
    return;
  }
  const int lane = tid & 63;
  const int slice = tile_slice[tile] + (tid >> 6);
  const uint4* slots = ell + (int64_t)slice_off[slice] * 64 + lane;
  const int nslots = slice_deg[slice];
  const float* Wto = W + L::layer(0) + L::L_TO;
  const float* Wfr = W + L::layer(0) + L::L_FROM;
  // ---- stage 2: per Phi module S, S', activity counts and their edge-feature moments
  v2f c_to[5], c_fr[5], m_to[15], m_fr[15];
  float mpt[D], mpf[D], tt[D], tf[D];
  {
    v2f Pi[5], dPi[5], S[5], Tj[5];
    ld5(T + L::T_B1_TO, Pi);
#pragma unroll
    for (int p = 0; p < 5; ++p) S[p] = Tj[p] = dPi[p] = c_to[p] = splat(0.f);
#pragma unroll
    for (int i = 0; i < 15; ++i) m_to[i] = splat(0.f);
    PHASE();
    mv2<D>(T + L::T_W1I_TO, x, Pi);
    const float deg_in = jr_pass_fwd<0, SLOT_IN>(slots, nslots, lds, doff, T + L::T_A_TO, Pi, S, Tj, c_to, m_to);
    PHASE();
    mv2<D>(T + L::T_W1I_TO, gx, dPi);
#pragma unroll
    for (int p = 0; p < 5; ++p) Tj[p] = __builtin_elementwise_fma(c_to[p], dPi[p], Tj[p]);   // S' = count (.) dPi + sum 1[z > 0] dPj
    const float* Sf = reinterpret_cast<const float*>(S);
    const float* Tf = reinterpret_cast<const float*>(Tj);
    const float* Pf_ = reinterpret_cast<const float*>(Pi);
#pragma unroll
    for (int i = 0; i < 5; ++i) reinterpret_cast<float2*>(Bn)[i] = make_float2(Pf_[2 * i], Pf_[2 * i + 1]);
    rec_group(r1 + 3 * 16, Sf, D, deg_in);
    rec_group(r2 + 3 * 16, Tf, D);
#pragma unroll
    for (int o = 0; o < D; ++o) mpt[o] = deg_in * Wto[L::PHI_B2 + o];
    PHASE();
    matvec10<D, true>(Wto + L::PHI_W2, D, 0, Sf, mpt);
    PHASE();
    matvec10<D, false>(Wto + L::PHI_W2, D, 0, Tf, tt);
  }
  PHASE();
  {
    v2f Pi[5], dPi[5], S[5], Tj[5];
    ld5(T + L::T_B1_FR, Pi);
#pragma unroll
    for (int p = 0; p < 5; ++p) S[p] = Tj[p] = dPi[p] = c_fr[p] = splat(0.f);
#pragma unroll
    for (int i = 0; i < 15; ++i) m_fr[i] = splat(0.f);
    PHASE();
    mv2<D>(T + L::T_W1I_FR, x, Pi);
    const float deg_out = jr_pass_fwd<D, SLOT_OUT>(slots, nslots, lds, doff, T + L::T_A_FR, Pi, S, Tj, c_fr, m_fr);
    PHASE();
    mv2<D>(T + L::T_W1I_FR, gx, dPi);
#pragma unroll
    for (int p = 0; p < 5; ++p) Tj[p] = __builtin_elementwise_fma(c_fr[p], dPi[p], Tj[p]);
    const float* Sf = reinterpret_cast<const float*>(S);
    const float* Tf = reinterpret_cast<const float*>(Tj);
    const float* Pf_ = reinterpret_cast<const float*>(Pi);
#pragma unroll
    for (int i = 0; i < 5; ++i) reinterpret_cast<float2*>(Bn + JR_BS)[i] = make_float2(Pf_[2 * i], Pf_[2 * i + 1]);
    rec_group(r1 + 4 * 16, Sf, D, deg_out);
    rec_group(r2 + 4 * 16, Tf, D);
#pragma unroll
    for (int o = 0; o < D; ++o) mpf[o] = deg_out * Wfr[L::PHI_B2 + o];
    PHASE();
    matvec10<D, true>(Wfr + L::PHI_W2, D, 0, Sf, mpf);
    PHASE();
    matvec10<D, false>(Wfr + L::PHI_W2, D, 0, Tf, tf);
  }
  // ---- node level: the statements of k_jr_node
  const float* Wu = W + L::layer(0) + L::L_UPD;
  const float* Wa = W + L::AL_W;
  float w[D], pq[P];
  load10(wv + n * D, w);
#pragma unroll
  for (int k = 0; k < P; ++k) pq[k] = prb[n * P + k];
  PHASE();
#define JR_NODE_BODY
#define JR_NODE_DIR(c)
#include "jr_node.h"
#undef JR_NODE_DIR
#undef JR_NODE_BODY
  // ---- the node's own edges: dS = W2^T cbar_mp (R1), dS' = W2^T chat_mp (R2); masked sums over the own edges = dS (.) count
  const float* cto = reinterpret_cast<const float*>(c_to);
  const float* cfr = reinterpret_cast<const float*>(c_fr);
  float dS[D], gt[D], gf[D];
  PHASE();
  matvecT<D, false>(Wto + L::PHI_W2, D, 0, ct, dS);
  store10(Bn + D, dS);
  {
    // groups 16..19 of R1: dS[o] * (attr moments), index o * 3 + c as in the W1 attr block; the in-edges carry the mirrored attr.
    // R2's right factors are tangents: no edge-feature part
    const float* mt = reinterpret_cast<const float*>(m_to);
    float mo[30];
#pragma unroll
    for (int o = 0; o < D; ++o) {
      gt[o] = dS[o] * cto[o];
      mo[o * 3] = -dS[o] * mt[o];
      mo[o * 3 + 1] = -dS[o] * mt[10 + o];
      mo[o * 3 + 2] = dS[o] * mt[20 + o];
    }
#pragma unroll
    for (int i = 0; i < 15; ++i) reinterpret_cast<float2*>(r1 + 16 * 16)[i] = make_float2(mo[2 * i], mo[2 * i + 1]);
  }
  PHASE();
  matvecT<D, false>(Wfr + L::PHI_W2, D, 0, cf, dS);
  store10(Bn + JR_BS + D, dS);
  {
    const float* mf = reinterpret_cast<const float*>(m_fr);
    float mo[34];
#pragma unroll
    for (int o = 0; o < D; ++o) {
      gf[o] = dS[o] * cfr[o];
      mo[o * 3] = dS[o] * mf[o];
      mo[o * 3 + 1] = dS[o] * mf[10 + o];
      mo[o * 3 + 2] = dS[o] * mf[20 + o];
    }
    mo[30] = mo[31] = mo[32] = mo[33] = 0.f;
#pragma unroll
    for (int i = 0; i < 17; ++i) reinterpret_cast<float2*>(r1 + 16 * 16 + 30)[i] = make_float2(mo[2 * i], mo[2 * i + 1]);
  }
  rec_group(r1 + 7 * 16, gt, D);
  rec_group(r1 + 8 * 16, gf, D);
  PHASE();
  matvecT<D, true>(Wto + L::PHI_W1, L::EIN, 0, gt, ch);
  PHASE();
  matvecT<D, true>(Wfr + L::PHI_W1, L::EIN, 0, gf, ch);
  store10(out + n * D, ch);
  PHASE();
  matvecT<D, false>(Wto + L::PHI_W2, D, 0, ct2, dS);
  store10(Bn + 2 * D, dS);
#pragma unroll
  for (int o = 0; o < D; ++o) gt[o] = dS[o] * cto[o];
  PHASE();
  matvecT<D, false>(Wfr + L::PHI_W2, D, 0, cf2, dS);
  store10(Bn + JR_BS + 2 * D, dS);
#pragma unroll
  for (int o = 0; o < D; ++o) gf[o] = dS[o] * cfr[o];
  rec_group(r2 + 7 * 16, gt, D);
  rec_group(r2 + 8 * 16, gf, D);
  rec_zero(r2, 16, ws::rec_f(false) / 16);
}

// ---------------------------------------------------------------------------------------------- pass B
// acc[o] += 1[z > 0] row[10 + o],  acc2[o] += 1[z > 0] row[20 + o],  z = row[o] + Pj[o] + AT . (flip a0, flip a1, a2),
// over the slots carrying MASK (attr signs as in fgnn_tile_vjp.hip's pass_rev)
template <unsigned MASK>
__device__ __forceinline__ void jr_pass_rev(const uint4* __restrict__ slots, int nslots, const float* __restrict__ lds,
                                            const float* __restrict__ AT, float flip, const v2f* Pj, v2f* acc, v2f* acc2) {
  v2f wa[15];
  ld_attr(AT, wa);
  for (SlotWalk<EDGE_PD, MASK> w(slots, nslots); w.more(); w.step())
    if (w.live()) {
      // (the chain of edge_preact, written out: through the helper k_jr_tile_b needs 108 VGPRs instead of 104 and ran 1 % slower)
      const uint4& c0 = w.slot();
      const v2f a0 = splat(flip * __uint_as_float(c0.y)), a1 = splat(flip * __uint_as_float(c0.z));
      const v2f a2 = splat(__uint_as_float(c0.w));
      const float* row = lds + w.row() * JR_BS;   // 120-byte rows: 8-byte aligned only
      v2f pi[5], ds[5], ds2[5], z[5];
      lds_row8(row, pi);
      lds_row8(row + D, ds);
      lds_row8(row + 2 * D, ds2);
#pragma unroll
      for (int p = 0; p < 5; ++p) z[p] = pi[p] + Pj[p];
#pragma unroll
      for (int p = 0; p < 5; ++p) z[p] = __builtin_elementwise_fma(wa[p], a0, z[p]);
#pragma unroll
      for (int p = 0; p < 5; ++p) z[p] = __builtin_elementwise_fma(wa[5 + p], a1, z[p]);
#pragma unroll
      for (int p = 0; p < 5; ++p) z[p] = __builtin_elementwise_fma(wa[10 + p], a2, z[p]);
#pragma unroll
      for (int p = 0; p < 5; ++p) {
        acc[p] += (v2f){z[p].x > 0.f ? ds[p].x : 0.f, z[p].y > 0.f ? ds[p].y : 0.f};
        acc2[p] += (v2f){z[p].x > 0.f ? ds2[p].x : 0.f, z[p].y > 0.f ? ds2[p].y : 0.f};
      }
    }
}

// lds: (n_t + n_h) x 120 bytes
template <int P>
__global__ __launch_bounds__(256) void k_jr_tile_b(int n_tiles, int chunk, int64_t N, const int32_t* __restrict__ tile_ptr,
                                                   const int32_t* __restrict__ tile_slice, const int32_t* __restrict__ halo,
                                                   const int32_t* __restrict__ halo_cnt, const int32_t* __restrict__ slice_off,
                                                   const uint8_t* __restrict__ slice_deg, const uint4* __restrict__ ell,
                                                   const float* __restrict__ W, int tofs, const float* __restrict__ h,
                                                   const float* __restrict__ B, float* __restrict__ out,
                                                   float* __restrict__ rec) {
  using L = WLayout<P>;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tile = xcd_tile_slot(chunk);
  if (tile >= n_tiles) return;
  const int tid = threadIdx.x;
  const int32_t t0 = tile_ptr[tile];
  const int n_t = tile_ptr[tile + 1] - t0;
  const int n_h = halo_cnt[tile];
  const int32_t* hl = halo + (int64_t)tile * HALO_CAP;
  const float* T = W + tofs;
  auto stage = [&](int half) {   // float2 units: 15 per half row
    for (int i = tid; i < (n_t + n_h) * (JR_BS / 2); i += TILE_THREADS) {
      const int row = i / (JR_BS / 2), c = i - row * (JR_BS / 2);
      const int64_t node = row < n_t ? (int64_t)(t0 + row) : (int64_t)hl[row - n_t];
      reinterpret_cast<float2*>(lds)[i] = reinterpret_cast<const float2*>(B + node * 2 * JR_BS)[half * (JR_BS / 2) + c];
    }
  };
  stage(0);
  __syncthreads();
  const bool active = tid < n_t;            // (every thread stays for the second staging pass and its barriers)
  const int64_t u = (int64_t)t0 + min(tid, n_t - 1);
  const int lane = tid & 63;
  const int slice = tile_slice[tile] + (min(tid, n_t - 1) >> 6);
  const uint4* slots = ell + (int64_t)slice_off[slice] * 64 + lane;
  const int nslots = active ? slice_deg[slice] : 0;
  float x[D];
  load10(h + u * D, x);
  v2f Pj[5], at[5], af[5], at2[5], af2[5];
#pragma unroll
  for (int p = 0; p < 5; ++p) Pj[p] = at[p] = af[p] = at2[p] = af2[p] = splat(0.f);
  // OUT slots: edge (u -> n) is an in-edge of n (Phi_to of n): { Pt, dS_to, dS'_to }[n] = first half row, attr = the slot's own
  // (T_A_TO holds the mirrored rows -> flip = -1 restores the plain attr weights)
  PHASE();
  mv2<D>(T + L::T_W1J_TO, x, Pj);
  jr_pass_rev<SLOT_OUT>(slots, nslots, lds, T + L::T_A_TO, -1.f, Pj, at, at2);
  __syncthreads();   // every wave is done with the first halves
  stage(1);
  __syncthreads();
  // IN slots: edge (n -> u) is an out-edge of n (Phi_from of n): second half row, attr = mirror of the slot's
#pragma unroll
  for (int p = 0; p < 5; ++p) Pj[p] = splat(0.f);
  PHASE();
  mv2<D>(T + L::T_W1J_FR, x, Pj);
  jr_pass_rev<SLOT_IN>(slots, nslots, lds, T + L::T_A_FR, -1.f, Pj, af, af2);
  if (!active) return;
  // neighbour-side cotangent sums: the W1j gradients are sum_u acc[u] (x) x[u] (R1) + acc'[u] (x) gbar[u] (R2)
  float* r1 = rec + u * ws::rec_f(false);
  float* r2 = rec + (N + u) * ws::rec_f(false);
  rec_group(r1 + 12 * 16, reinterpret_cast<const float*>(at), D);
  rec_group(r1 + 13 * 16, reinterpret_cast<const float*>(af), D);
  rec_group(r2 + 12 * 16, reinterpret_cast<const float*>(at2), D);
  rec_group(r2 + 13 * 16, reinterpret_cast<const float*>(af2), D);
  float g[D];
  load10(out + u * D, g);
  PHASE();
  matvecT<D, true>(W + L::layer(0) + L::L_TO + L::PHI_W1, L::EIN, D, reinterpret_cast<const float*>(at), g);
  PHASE();
  matvecT<D, true>(W + L::layer(0) + L::L_FROM + L::PHI_W1, L::EIN, D, reinterpret_cast<const float*>(af), g);
  store10(out + u * D, g);
}

// ---------------------------------------------------------------------------------------------- host
// Dynamic LDS beyond 64 KB has to be granted per device before the first launch.
static bool jr_tile_lds_granted(int want_a, int want_b) {
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return false;
  static int state[64] = {0};   // 0 unknown, 1 granted, -1 refused
  if (state[dev] == 0) {
    const bool ok = hipFuncSetAttribute((const void*)k_jr_tile_a<2>, hipFuncAttributeMaxDynamicSharedMemorySize, want_a) == hipSuccess &&
                    hipFuncSetAttribute((const void*)k_jr_tile_b<2>, hipFuncAttributeMaxDynamicSharedMemorySize, want_b) == hipSuccess;
    if (!ok) (void)hipGetLastError();
    state[dev] = ok ? 1 : -1;
  }
  return state[dev] > 0;
}

int psignn_jr_tiled_ok(const psignn_plan* p, int nl) {
  return p && p->tiled && !p->mixed && nl == 1 && p->max_rows <= TILE_MAX + HALO_CAP;
}

// h, prb, v, gbar, out_h in PLAN order.  B: (N, 60) floats; rec: (2 N, 320) = R1 then R2, every group written.
int psignn_jr_tile_records(const psignn_plan* p, const float* W, const float* h, const float* prb, const float* v,
                           const float* gbar, float* out_h, float* B, float* rec, hipStream_t st) {
  ARG_CHECK(psignn_jr_tiled_ok(p, 1), "tiled backward of the VJP: tiled plans of the dirichlet family");
  using L = WLayout<2>;
  const int64_t N = p->N;
  const int chunk = (int)cdiv(p->n_tiles, 8);
  const unsigned grid = (unsigned)(chunk * 8);
  const size_t lds_a = (size_t)p->max_rows * 2 * JR_RS * 4;
  const size_t lds_b = (size_t)p->max_rows * JR_BS * 4;
  constexpr int cap_a = (TILE_MAX + HALO_CAP) * 2 * JR_RS * 4, cap_b = (TILE_MAX + HALO_CAP) * JR_BS * 4;   // 120 KB, 90 KB
  if (lds_a > 64 * 1024 || lds_b > 64 * 1024)
    ARG_CHECK(jr_tile_lds_granted(cap_a, cap_b), "the device refused the dynamic LDS of the tiled backward of the VJP");
  const int tofs = L::tp_layer(1, false, 0);
  // pass A reads h, gbar, v (40 N each), prb (8 N), flags, writes B (240 N), the node-local d phi / d h (40 N) and the two
  // records less their groups 12, 13 (2 x 1 152 N); 20 bytes per directed edge (slot + attr)
  PROF_BYTES((int64_t)N * (129 + 240 + 40 + 2 * (ws::rec_f(false) - 32) * 4) + 20 * p->Ep);
  LAUNCH("k_jr_tile_a", st, (k_jr_tile_a<2><<<grid, TILE_THREADS, lds_a, st>>>(
      (int)p->n_tiles, chunk, N, PLAN_TILES_FLAGS(p), W, tofs, h, prb, v, gbar, B, out_h, rec)));
  // pass B reads h (40 N), B (240 N) and the partial d phi / d h (40 N), writes it (40 N) and groups 12, 13 of both records
  // (256 N); 20 bytes per directed edge
  PROF_BYTES((int64_t)N * (40 + 240 + 40 + 40 + 256) + 20 * p->Ep);
  LAUNCH("k_jr_tile_b", st, (k_jr_tile_b<2><<<grid, TILE_THREADS, lds_b, st>>>(
      (int)p->n_tiles, chunk, N, PLAN_TILES(p), W, tofs, h, B, out_h, rec)));
  HIP_TRY(hipGetLastError());
  return PSIGNN_OK;
}
