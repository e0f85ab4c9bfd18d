// Linearised GNN block for Newton-Krylov (BASELINE config 5: 1M nodes, GMRES on J_f(h) - I; SURVEY section 8a "JVP needed for
// config 5 ... dm_e = W2(1[z>0] (W1i v_i + W1j v_j)) ...", section 8d "B_jvp (+ N 40 if h-dependent masks are recomputed rather
// than stored)").  One Newton step runs tens of GMRES iterations at a FIXED state h: every J_f(h) v of those re-derives, in
// k_jvp_tile, the whole value path of f -- pre-activations of 12 M edge directions, gate, update MLP, LayerNorm statistics -- only
// to obtain the relu masks and a few per-node scalars, which do not depend on v.  Here they are computed once per Newton step and
// stored (psignn_lin_build), and the product is the LINEAR operator they define (psignn_lin_jvp):
//
//   per slot row s (one ELL row of one 64-lane slice) and lane l, ONE dword instead of the 16-byte slot record:
//     slot[s][l] = LDS row of the neighbour (bits 0..9; 0 for an empty slot, whose masks are 0)
//                | 1[slot carries an in-edge  and z_to[o]   > 0] << (10 + o)      o < 10   (Phi_to pre-activations)
//                | 1[slot carries an out-edge and z_from[o] > 0] << (20 + o)               (Phi_from)
//   per node (24 floats): alpha, alpha (1 - alpha), 1 / sqrt(var + eps), bit mask of the update MLP's hidden relu, update[10], y_hat[10]
//
//   J v = LN'( v + alpha (1 - alpha) (w_a . dc) update + alpha U2 (1[q>0] (U1 dc)) ),  dc = [v, G_to dS_to, G_fr dS_fr],
//   dS_dir[o] = sum over the node's slots of mask (dPi_dir[o] + dPj_dir[o]),  dP = W1 v  (second Phi layer folded as in k_f_tile)
//
// Against k_jvp_tile at 1M nodes: ~0.4 x the VALU instructions per wave, 80-byte LDS rows (tangent projections only: six
// workgroups per CU instead of three), about the same bytes (the 96-byte node record replaces the h row, the 16-byte slot records
// shrink to 4 bytes).  Dirichlet plans with a single-layer block; mixed plans by default: the tiles WITHOUT Neumann nodes (all but the
// boundary tiles) go through the stored linearisation, the few tiles holding Neumann nodes through k_jvp_tile at the state kept from
// the build; with the Neumann rows stored (below) every tile goes through the stored form.
//
// Transposed product (psignn_lin_vjp, k_vjp_lin): out = J_f(h)^T w from the SAME masks and node records, so that it is the exact
// transpose of psignn_lin_jvp (masks recomputed from projections could flip where a pre-activation is ~0).  Per node n, the node-local
// backward through LN', the update MLP (stored hidden mask) and the gate gives the direct term and c[n] = [c_to | c_fr], the
// cotangents of dS_to / dS_fr (0 on Dirichlet rows, which are copies of H_init); then
//   out[u] = direct[u] + W1i_to^T (cnt_to[u] . c_to[u]) + W1i_fr^T (cnt_fr[u] . c_fr[u])
//          + W1j_to^T sum_{slots of u -> n} m_to(n's slot of the pair) . c_to[n] + W1j_fr^T sum m_fr(n's slot of the pair) . c_fr[n]
// cnt_dir[u][o] = number of u's slots with mask bit o set (c[u] is the same on all of them: a popcount, as pass A of the tiled VJP).
// The neighbour masks live with the receiving node n, so the handle keeps a transposed slot-dword array aligned with `slot`:
//   tslot[s][l] = u's LDS row field of the slot | n's Phi_to masks of edge u -> n (bits 10..19) | n's Phi_from masks of n -> u (20..29)
// filled per build by k_lin_tfill through a reverse slot map (k_lin_rev, once per handle, on the device from the plan's ELL rows),
// matched per edge direction: the Phi_to and Phi_from masks of one pair may come from two different slots of n's row.
// Both arrays are allocated on the first psignn_lin_vjp: the build and psignn_lin_jvp do not change.  One launch per product:
// stage 1 computes c for the tile and halo rows into 80-byte LDS rows (halo rows recomputed per tile), stage 2 walks the slots from
// u's side (a gather: fixed order, no atomics, bitwise reproducible).  Mixed plans: the tiled VJP at the state kept by the build.
//
// Neumann rows stored (psignn_lin_create_opts(.., neumann_stored = 1), mixed plans, opt-in): a Neumann row is REPLACED by
// LayerNorm(update_neumann([h, Phi_neumann(h), prb, normal])) (mixed/psignn/model.py:225,233-236,241 of the reference), so its
// Phi_to / Phi_from masks are never used and Phi_neumann sums over the row's OUT edges -- the edge set of Phi_from.  No third mask
// set is needed: the row keeps Phi_neumann's first-layer relu masks in the Phi_from bit field of its slot dwords (Phi_to bits 0) and
// {1 / sqrt(var + eps), hidden relu mask of update_neumann, y_hat[10]} in its 24-float record; which rows are Neumann rows comes from
// the plan's node flags.  Then every tile goes through the stored form and the handle keeps no copy of the state:
//   build   k_lin_build<3> on the plan's first tile group, k_lin_build<3, true> on the tiles holding Neumann nodes (144-byte LDS
//           rows [Pj_to | Pj_from | Pj_neu | pad]; the Neumann branch repeats k_jvp_tile's value path operation by operation)
//   J v     k_jvp_lin<3> / k_jvp_lin<3, true> on the same two groups:  J v [n] = LN'( N2 (1[q > 0] (N1h v_n + G_n dS_n)) ),
//           dS_n = sum over n's OUT slots of mask (W1i_neu v_n + W1j_neu v_u); only the second group pays for the third LDS column
//   J^T w   k_vjp_lin_mixed<3>, ONE launch; per tile the plain or the Neumann form by "a Neumann row among the tile's own and HALO
//           rows" (a tile without Neumann nodes of its own still receives c_neu of a halo row): c[n] = [0 | c_neu[n]] keeps the 80-byte LDS rows; bit 30 of a
//           transposed slot dword marks a Neumann partner (k_lin_rev<true>), whose masked c_neu goes to a third sum, applied through
//           W1j_neu^T; a Neumann row's own side is W1i_neu^T (cnt . c_neu).  The tile list is made once per handle (k_lin_vgroup + the
//           host), Neumann tiles on the first workgroups.
// Every kernel instantiation that exists without the option is unchanged (NEU = false is the code as it was).
//
// weight loads of mv2 pinned chunk by chunk (tile_helpers.h; A/B in profiles/r3_ab_mv2.txt: k_jvp_lin 53 -> 48.5 us)
#define MV2_LAUNDER 2
#include "tile_helpers.h"
#include "internal.h"
#include <stdlib.h>
#include <string.h>

#define LIN_REC 24            // floats per node record
#define LIN_CHUNK 8           // slot dwords requested at once by the product kernel (a slice has ~6 slot rows)

struct psignn_lin {
  const psignn_plan* plan = nullptr;
  uint32_t* slot = nullptr;     // (ell_rows, 64)
  float* rec = nullptr;         // (N, LIN_REC)
  float *h = nullptr, *prb = nullptr, *nrm = nullptr;   // mixed plans: the state of the last build (k_jvp_tile on the Neumann tiles)
  size_t bytes = 0;
  int built = 0;
  // transposed product (dirichlet plans), allocated on the first psignn_lin_vjp: the build and psignn_lin_jvp never touch them
  mutable int2* rev = nullptr;        // (ell_rows, 64) reverse slot map per edge direction, filled once
  mutable uint32_t* tslot = nullptr;  // (ell_rows, 64) transposed slot dwords, masks re-filled once per build
  mutable int tfilled = 0;            // tslot holds the masks of the last build
  mutable size_t tbytes = 0;
  // mixed plans, Neumann rows stored (psignn_lin_create_opts): no state copies; the transposed product's tile groups
  int neu = 0;
  int32_t* vlist = nullptr;           // (8 cdiv(n_tiles, 8)) tile list of k_vjp_lin_mixed
  int n_vplain = 0;                   // tiles without a Neumann row among tile + halo
};
#define LIN_RS_NEU 36         // floats per LDS row of the tiles holding Neumann nodes: [Pj_to | Pj_from | Pj_neu | pad 6].  A
                              // ds_read_b128 is served over 16 slots of 16 bytes: a 144-byte row starts on slot 9 r mod 16, an odd
                              // stride -- sixteen consecutive rows on sixteen different slots, as the 80-byte rows (5 r mod 16); the
                              // 120-byte payload unpadded would misalign the b128 reads and 128 bytes put every row on slot 0

// Stage 1 of both kernels: rows [Pj_to | Pj_from] = W1j_{to,from} src[node] of the tile's own and halo nodes -> 80-byte LDS rows
// (own row by its lane; halo rows as HALF rows over all four waves, as in k_f_tile).  Returns the lane's own src row in x.
// NEU: 144-byte rows with a third column Pj_neu = W1j_neu src[node] (the Phi_neumann projection a Neumann row's OUT slots read)
template <int P, bool NEU = false>
__device__ __forceinline__ void lin_stage1(const float* __restrict__ T, const float* __restrict__ src, const int32_t t0, const int n_t,
                                           const int n_h, const int32_t* __restrict__ hl, float* __restrict__ lds, float* x,
                                           const float* __restrict__ TN = nullptr) {
  using L = WLayout<P>;
  constexpr int RS = NEU ? LIN_RS_NEU : 20;
  const int tid = threadIdx.x;
  const int32_t hidx_w = (tid >> 6 & 1) * 64 + (tid & 63);
  int32_t hnode = 0;
  if (hidx_w < n_h) hnode = hl[hidx_w];
  float xr[D], xh[D];
  if (tid < n_t) load10(src + (int64_t)(t0 + tid) * D, xr);
  if (hidx_w < n_h) load10(src + (int64_t)hnode * D, xh);
  if (tid < n_t) {
#pragma unroll
    for (int o = 0; o < D; ++o) x[o] = xr[o];
    v2f ta[5], tb[5];
#pragma unroll
    for (int p = 0; p < 5; ++p) ta[p] = tb[p] = splat(0.f);
    PHASE();
    mv2<D>(T + L::T_W1J_TO, xr, ta);
    PHASE();
    mv2<D>(T + L::T_W1J_FR, xr, tb);
    float4* q = reinterpret_cast<float4*>(lds + tid * RS);
    q[0] = make_float4(ta[0].x, ta[0].y, ta[1].x, ta[1].y);
    q[1] = make_float4(ta[2].x, ta[2].y, ta[3].x, ta[3].y);
    q[2] = make_float4(ta[4].x, ta[4].y, tb[0].x, tb[0].y);
    q[3] = make_float4(tb[1].x, tb[1].y, tb[2].x, tb[2].y);
    q[4] = make_float4(tb[3].x, tb[3].y, tb[4].x, tb[4].y);
  }
  if constexpr (NEU) {   // third column of the own and the halo rows, one row per thread
    for (int row = tid; row < n_t + n_h; row += TILE_THREADS) {
      float xq[D];
      load10(src + (row < n_t ? (int64_t)(t0 + row) : (int64_t)hl[row - n_t]) * D, xq);
      v2f tc[5];
#pragma unroll
      for (int p = 0; p < 5; ++p) tc[p] = splat(0.f);
      PHASE();
      mv2<D>(TN + L::N_W1J, xq, tc);
      float4* q = reinterpret_cast<float4*>(lds + row * RS + 2 * D);
      q[0] = make_float4(tc[0].x, tc[0].y, tc[1].x, tc[1].y);
      q[1] = make_float4(tc[2].x, tc[2].y, tc[3].x, tc[3].y);
      reinterpret_cast<float2*>(q + 2)[0] = make_float2(tc[4].x, tc[4].y);
    }
  }
  const int half = __builtin_amdgcn_readfirstlane(tid >> 7);   // 0: Phi_to columns, 1: Phi_from columns
  for (int hb = 0; hb < n_h; hb += 128) {
    const int idx = hb + hidx_w;
    if (hb > 0 && idx < n_h) hnode = hl[idx];
    if (idx < n_h) {
      float xq[D];
      if (hb == 0) {
#pragma unroll
        for (int o = 0; o < D; ++o) xq[o] = xh[o];
      } else {
        load10(src + (int64_t)hnode * D, xq);
      }
      v2f ta[5];
#pragma unroll
      for (int p = 0; p < 5; ++p) ta[p] = splat(0.f);
      PHASE();
      float* rowp = lds + (n_t + idx) * RS;
      if (half == 0) {
        mv2<D>(T + L::T_W1J_TO, xq, ta);
        float4* q = reinterpret_cast<float4*>(rowp);
        q[0] = make_float4(ta[0].x, ta[0].y, ta[1].x, ta[1].y);
        q[1] = make_float4(ta[2].x, ta[2].y, ta[3].x, ta[3].y);
        reinterpret_cast<float2*>(rowp + 8)[0] = make_float2(ta[4].x, ta[4].y);
      } else {
        mv2<D>(T + L::T_W1J_FR, xq, ta);
        reinterpret_cast<float2*>(rowp + 10)[0] = make_float2(ta[0].x, ta[0].y);
        float4* q = reinterpret_cast<float4*>(rowp + 12);
        q[0] = make_float4(ta[1].x, ta[1].y, ta[2].x, ta[2].y);
        q[1] = make_float4(ta[3].x, ta[3].y, ta[4].x, ta[4].y);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------
// Build: the value path of f at h (same formulas and operation order as k_jvp_tile's value half), storing what J_f(h) needs.
// ------------------------------------------------------------------------------------------------------------------
// NEU (the tiles of a mixed plan that hold Neumann nodes, handles that store the Neumann rows): 144-byte LDS rows with the
// Phi_neumann column; a Neumann row stores the relu masks of Phi_neumann's first layer on its OUT slots in the Phi_from bit field
// (Phi_to bits 0: the row is REPLACED by LayerNorm(update_neumann(..)), its Phi_to / Phi_from sums are never used) and the record
// {0, 0, 1 / sqrt(var + eps), hidden relu mask of update_neumann, 0 x 10, y_hat[10]} -- the value path of k_jvp_tile's Neumann branch.
template <int P, bool NEU = false>
__global__ __launch_bounds__(TILE_THREADS) void k_lin_build(int n_tiles, int chunk, const int32_t* __restrict__ tile_list, const TileCtx C,
                                                            const float* __restrict__ W,
                                                            int lofs, int tofs, const float* __restrict__ h,
                                                            const float* __restrict__ prb, uint32_t* __restrict__ slot,
                                                            float* __restrict__ rec, int tnofs = 0,
                                                            const float* __restrict__ nrm = nullptr) {
  using L = WLayout<P>;
  constexpr int RS = NEU ? LIN_RS_NEU : 20;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int slot_ = xcd_tile_slot(chunk);
  if (slot_ >= n_tiles) return;
  const int tile = tile_list ? tile_list[slot_] : slot_;   // mixed plans: the tiles without Neumann nodes
  const int tid = threadIdx.x;
  const int tn = C.tile_nodes;
  const int32_t t0 = tn ? tile * tn : C.tile_ptr[tile];
  const int n_t = tn ? min(tn, C.n_nodes - t0) : C.tile_ptr[tile + 1] - t0;
  const int n_h = C.halo_cnt[tile];
  const int32_t* hl = C.halo + (int64_t)tile * HALO_CAP;
  const float* T = W + tofs;
  float x[D];
#pragma unroll
  for (int o = 0; o < D; ++o) x[o] = 0.f;
  lin_stage1<P, NEU>(T, h, t0, n_t, n_h, hl, lds, x, W + tnofs);
  __syncthreads();
  if (tid >= n_t) return;
  const int lane = tid & 63;
  const int64_t n = (int64_t)t0 + tid;
  const uint8_t fl = C.flags_p[n];
  if (fl & FLAG_DIRICHLET) return;   // (the product kernel writes zeros for such a row without looking at its slots)
  const int slice = __builtin_amdgcn_readfirstlane((tn ? tile * (tn >> 6) : C.tile_slice[tile]) + (tid >> 6));
  const int srow0 = C.slice_off[slice];
  const int nslots = C.slice_deg[slice];
  const uint4* slots = C.ell + (int64_t)srow0 * 64 + lane;
  uint32_t* so = slot + (int64_t)srow0 * 64 + lane;
  if constexpr (NEU) {
    if (fl & FLAG_NEUMANN) {
      // ---- Neumann row: y = N2 relu(q) + nb2, q = nb1 + deg gN + N1h x + Gn S_n + N1p [prb | normal]; formulas and operation
      // order of k_jvp_tile's Neumann branch (edge_pass_jvp: z = Pi + Pj, then the three attr fmas)
      const float* TN = W + tnofs;
      v2f Pi[5], S_n[5], wa[15];
      ld5(TN + L::N_B1, Pi);
#pragma unroll
      for (int p = 0; p < 5; ++p) S_n[p] = splat(0.f);
      PHASE();
      mv2<D>(TN + L::N_W1I, x, Pi);
#pragma unroll
      for (int i = 0; i < 15; ++i) wa[i] = reinterpret_cast<const v2f*>(TN + L::N_A)[i];
      float deg_out = 0.f;
      for (int r = 0; r < nslots; ++r) {
        const uint4 c0 = slots[(int64_t)r * 64];
        const unsigned w = c0.x;
        unsigned word = 0;
        if ((w & 0xFFFFu) != ELL_EMPTY) {
          word = w & 0xFFFFu;
          if (w & SLOT_OUT) {
            const v2f a0 = splat(__uint_as_float(c0.y)), a1 = splat(__uint_as_float(c0.z)), a2 = splat(__uint_as_float(c0.w));
            const float4* rp = reinterpret_cast<const float4*>(lds + (int)word * RS + 2 * D);
            const float4 v0 = rp[0], v1 = rp[1];
            const float2 v2 = reinterpret_cast<const float2*>(rp + 2)[0];
            v2f z[5] = {(v2f){v0.x, v0.y}, (v2f){v0.z, v0.w}, (v2f){v1.x, v1.y}, (v2f){v1.z, v1.w}, (v2f){v2.x, v2.y}};
            deg_out += 1.f;
#pragma unroll
            for (int p = 0; p < 5; ++p) z[p] = Pi[p] + z[p];
#pragma unroll
            for (int p = 0; p < 5; ++p) z[p] = __builtin_elementwise_fma(wa[p], a0, z[p]);
#pragma unroll
            for (int p = 0; p < 5; ++p) z[p] = __builtin_elementwise_fma(wa[5 + p], a1, z[p]);
#pragma unroll
            for (int p = 0; p < 5; ++p) z[p] = __builtin_elementwise_fma(wa[10 + p], a2, z[p]);
#pragma unroll
            for (int p = 0; p < 5; ++p) {
              S_n[p] += __builtin_elementwise_max(z[p], splat(0.f));
              word |= (z[p].x > 0.f ? 1u : 0u) << (20 + 2 * p);
              word |= (z[p].y > 0.f ? 1u : 0u) << (21 + 2 * p);
            }
          }
        }
        so[(int64_t)r * 64] = word;
      }
      v2f q[5], gN[5], y2[5];
      ld5(TN + L::N_NB1, q);
      ld5(TN + L::N_gN, gN);
#pragma unroll
      for (int p = 0; p < 5; ++p) q[p] = __builtin_elementwise_fma(splat(deg_out), gN[p], q[p]);
      PHASE();
      mv2<D>(TN + L::N_N1H, x, q);
      PHASE();
      mv2<D>(TN + L::N_GN, reinterpret_cast<const float*>(S_n), q);
      float pq[P + 2];
#pragma unroll
      for (int k = 0; k < P; ++k) pq[k] = prb[n * P + k];
      pq[P] = nrm[n * 2];
      pq[P + 1] = nrm[n * 2 + 1];
      PHASE();
      mv2<P + 2>(TN + L::N_N1P, pq, q);
      unsigned hm = 0;
#pragma unroll
      for (int p = 0; p < 5; ++p) {
        hm |= (q[p].x > 0.f ? 1u : 0u) << (2 * p);
        hm |= (q[p].y > 0.f ? 1u : 0u) << (2 * p + 1);
        q[p] = __builtin_elementwise_max(q[p], splat(0.f));
      }
      ld5(TN + L::N_NB2, y2);
      PHASE();
      mv2<D>(TN + L::N_N2, reinterpret_cast<const float*>(q), y2);
      const float* y = reinterpret_cast<const float*>(y2);
      float mu = 0.f;
#pragma unroll
      for (int o = 0; o < D; ++o) mu += y[o];
      mu *= (1.f / D);
      float var = 0.f;
#pragma unroll
      for (int o = 0; o < D; ++o) {
        const float c = y[o] - mu;
        var = fmaf(c, c, var);
      }
      var *= (1.f / D);
      const float rs = 1.f / sqrtf(var + 1e-5f);
      float yh[D];
#pragma unroll
      for (int o = 0; o < D; ++o) yh[o] = (y[o] - mu) * rs;
      float4* rp = reinterpret_cast<float4*>(rec + n * LIN_REC);
      rp[0] = make_float4(0.f, 0.f, rs, __uint_as_float(hm));
      rp[1] = rp[2] = make_float4(0.f, 0.f, 0.f, 0.f);
      rp[3] = make_float4(0.f, 0.f, yh[0], yh[1]);
      rp[4] = make_float4(yh[2], yh[3], yh[4], yh[5]);
      rp[5] = make_float4(yh[6], yh[7], yh[8], yh[9]);
      return;
    }
  }
  // ---- neighbour sums and masks
  v2f S_to[5], S_fr[5], pt[5], pf[5], wt[15], wf[15];
  {
    v2f Pi[5], Pi2[5];
    ld5(T + L::T_B1_TO, Pi);
    ld5(T + L::T_B1_FR, Pi2);
    PHASE();
    mv2<D>(T + L::T_W1I_TO, x, Pi);
    PHASE();
    mv2<D>(T + L::T_W1I_FR, x, Pi2);
    const v2f sc = splat(RELU_SCALE);
#pragma unroll
    for (int p = 0; p < 5; ++p) {
      pt[p] = Pi[p] * sc;
      pf[p] = Pi2[p] * sc;
      S_to[p] = S_fr[p] = splat(0.f);
    }
#pragma unroll
    for (int i = 0; i < 15; ++i) {
      wt[i] = reinterpret_cast<const v2f*>(T + L::T_A_TO)[i];
      wf[i] = reinterpret_cast<const v2f*>(T + L::T_A_FR)[i];
    }
  }
  float deg_in = 0.f, deg_out = 0.f;
  const v2f sc = splat(RELU_SCALE);
  uint4 c0 = nslots > 0 ? slots[0] : make_uint4(ELL_EMPTY, 0u, 0u, 0u);
  for (int r = 0; r < nslots; ++r) {
    const uint4 nx = slots[(int64_t)min(r + 1, nslots - 1) * 64];
    const unsigned w = c0.x;
    unsigned word = 0;
    if ((w & 0xFFFFu) != ELL_EMPTY) {
      word = w & 0xFFFFu;
      const v2f a01 = (v2f){__uint_as_float(c0.y), __uint_as_float(c0.z)} * sc;
      const v2f a2 = (v2f){__uint_as_float(c0.w) * RELU_SCALE, 0.f};
      const float4* rp = reinterpret_cast<const float4*>(lds + (int)word * RS);
      const float4 v0 = rp[0], v1 = rp[1], v2 = rp[2], v3 = rp[3], v4 = rp[4];
      if (w & SLOT_IN) {
        v2f z[5] = {(v2f){v0.x, v0.y}, (v2f){v0.z, v0.w}, (v2f){v1.x, v1.y}, (v2f){v1.z, v1.w}, (v2f){v2.x, v2.y}};
        deg_in += 1.f;
#pragma unroll
        for (int p = 0; p < 5; ++p) z[p] = __builtin_elementwise_fma(z[p], sc, pt[p]);
#pragma unroll
        for (int p = 0; p < 5; ++p) z[p] = pk_fma_lo(wt[p], a01, z[p]);
#pragma unroll
        for (int p = 0; p < 5; ++p) z[p] = pk_fma_hi(wt[5 + p], a01, z[p]);
#pragma unroll
        for (int p = 0; p < 5; ++p) z[p] = pk_fma_lo_clamp(wt[10 + p], a2, z[p]);
#pragma unroll
        for (int p = 0; p < 5; ++p) {   // clamp(2^-40 z) > 0  <=>  z > 0, as k_jvp_tile's mask
          S_to[p] += z[p];
          word |= (z[p].x > 0.f ? 1u : 0u) << (10 + 2 * p);
          word |= (z[p].y > 0.f ? 1u : 0u) << (11 + 2 * p);
        }
      }
      if (w & SLOT_OUT) {
        v2f z[5] = {(v2f){v2.z, v2.w}, (v2f){v3.x, v3.y}, (v2f){v3.z, v3.w}, (v2f){v4.x, v4.y}, (v2f){v4.z, v4.w}};
        deg_out += 1.f;
#pragma unroll
        for (int p = 0; p < 5; ++p) z[p] = __builtin_elementwise_fma(z[p], sc, pf[p]);
#pragma unroll
        for (int p = 0; p < 5; ++p) z[p] = pk_fma_lo(wf[p], a01, z[p]);
#pragma unroll
        for (int p = 0; p < 5; ++p) z[p] = pk_fma_hi(wf[5 + p], a01, z[p]);
#pragma unroll
        for (int p = 0; p < 5; ++p) z[p] = pk_fma_lo_clamp(wf[10 + p], a2, z[p]);
#pragma unroll
        for (int p = 0; p < 5; ++p) {
          S_fr[p] += z[p];
          word |= (z[p].x > 0.f ? 1u : 0u) << (20 + 2 * p);
          word |= (z[p].y > 0.f ? 1u : 0u) << (21 + 2 * p);
        }
      }
    }
    so[(int64_t)r * 64] = word;
    c0 = nx;
  }
  const v2f us = splat(RELU_UNSCALE);
#pragma unroll
  for (int p = 0; p < 5; ++p) {
    S_to[p] *= us;
    S_fr[p] *= us;
  }
  // ---- gate and update MLP (second Phi layer folded), LayerNorm statistics: as k_jvp_tile
  const float* Wf = W + lofs + L::L_FOLD;
  const float* Wa = W + L::AL_W;
  const float* sto = reinterpret_cast<const float*>(S_to);
  const float* sfr = reinterpret_cast<const float*>(S_fr);
  float pq[P];
#pragma unroll
  for (int k = 0; k < P; ++k) pq[k] = prb[n * P + k];
  PHASE();
  float al = fmaf(deg_in, Wf[L::F_ABTO], fmaf(deg_out, Wf[L::F_ABFR], W[L::AL_B]));
#pragma unroll
  for (int k = 0; k < D; ++k) al = fmaf(Wa[k], x[k], al);
#pragma unroll
  for (int k = 0; k < D; ++k) al = fmaf(Wf[L::F_ATO + k], sto[k], al);
#pragma unroll
  for (int k = 0; k < D; ++k) al = fmaf(Wf[L::F_AFR + k], sfr[k], al);
#pragma unroll
  for (int k = 0; k < P; ++k) al = fmaf(Wa[3 * D + k], pq[k], al);
  al = 1.f / (1.f + expf(-al));
  v2f q[5], g1[5], g2[5], upd[5];
  ld5(T + L::T_HB, q);
  ld5(T + L::T_gTO, g1);
  ld5(T + L::T_gFR, g2);
#pragma unroll
  for (int p = 0; p < 5; ++p)
    q[p] = __builtin_elementwise_fma(splat(deg_in), g1[p], __builtin_elementwise_fma(splat(deg_out), g2[p], q[p]));
  PHASE();
  mv2<D>(T + L::T_U1H, x, q);
  PHASE();
  mv2<D>(T + L::T_GTO, sto, q);
  PHASE();
  mv2<D>(T + L::T_GFR, sfr, q);
  mv2<P>(T + L::T_U1P, pq, q);
  unsigned hm = 0;
#pragma unroll
  for (int p = 0; p < 5; ++p) {
    hm |= (q[p].x > 0.f ? 1u : 0u) << (2 * p);
    hm |= (q[p].y > 0.f ? 1u : 0u) << (2 * p + 1);
    q[p] = __builtin_elementwise_max(q[p], splat(0.f));
  }
  ld5(T + L::T_C2, upd);
  PHASE();
  mv2<D>(T + L::T_U2, reinterpret_cast<const float*>(q), upd);
  const float* u = reinterpret_cast<const float*>(upd);
  float y[D], mu = 0.f;
#pragma unroll
  for (int o = 0; o < D; ++o) {
    y[o] = fmaf(al, u[o], x[o]);
    mu += y[o];
  }
  mu *= (1.f / D);
  float var = 0.f;
#pragma unroll
  for (int o = 0; o < D; ++o) {
    const float c = y[o] - mu;
    var = fmaf(c, c, var);
  }
  var *= (1.f / D);
  const float rs = 1.f / sqrtf(var + 1e-5f);
  float4* rp = reinterpret_cast<float4*>(rec + n * LIN_REC);
  float yh[D];
#pragma unroll
  for (int o = 0; o < D; ++o) yh[o] = (y[o] - mu) * rs;
  rp[0] = make_float4(al, al * (1.f - al), rs, __uint_as_float(hm));
  rp[1] = make_float4(u[0], u[1], u[2], u[3]);
  rp[2] = make_float4(u[4], u[5], u[6], u[7]);
  rp[3] = make_float4(u[8], u[9], yh[0], yh[1]);
  rp[4] = make_float4(yh[2], yh[3], yh[4], yh[5]);
  rp[5] = make_float4(yh[6], yh[7], yh[8], yh[9]);
}

// ------------------------------------------------------------------------------------------------------------------
// Product: out = J_f(h) v from the stored linearisation
// ------------------------------------------------------------------------------------------------------------------
// Wave priorities per phase as in k_f_tile were measured and removed (profiles/r3_ab_prio_jvp.txt): k_jvp_lin 49.2 -> 50.7 us.
// NEU (tiles holding Neumann nodes, Neumann rows stored): a Neumann row's walk sums its Phi_from bit field over the third LDS column,
//   J v = LN'( N2 (1[q > 0] (N1h v_n + G_n dS_n)) ),  dS_n = sum over the OUT slots of mask (W1i_neu v_n + W1j_neu v_u)
template <int P, bool NEU = false>
__global__ __launch_bounds__(TILE_THREADS) void k_jvp_lin(int n_tiles, int chunk, const int32_t* __restrict__ tile_list,
                                                                  const TileCtx C, const float* __restrict__ W,
                                                                  int lofs, int tofs, const uint32_t* __restrict__ slot,
                                                                  const float* __restrict__ rec,
                                                                  const float* __restrict__ tv, float* __restrict__ out,
                                                                  int tnofs = 0) {
  using L = WLayout<P>;
  constexpr int RS = NEU ? LIN_RS_NEU : 20;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int slot_ = xcd_tile_slot(chunk);
  if (slot_ >= n_tiles) return;
  const int tile = tile_list ? tile_list[slot_] : slot_;
  const int tid = threadIdx.x;
  const int tn = C.tile_nodes;
  const int32_t t0 = tn ? tile * tn : C.tile_ptr[tile];
  const int n_t = tn ? min(tn, C.n_nodes - t0) : C.tile_ptr[tile + 1] - t0;
  const int n_h = C.halo_cnt[tile];
  const int32_t* hl = C.halo + (int64_t)tile * HALO_CAP;
  const float* T = W + tofs;
  float dx[D];
  lin_stage1<P, NEU>(T, tv, t0, n_t, n_h, hl, lds, dx, W + tnofs);
  __syncthreads();
  if (tid >= n_t) return;
  const int64_t n = (int64_t)t0 + tid;
  float dy[D];
  const uint8_t fl = C.flags_p[n];
  if (fl & FLAG_DIRICHLET) {
#pragma unroll
    for (int o = 0; o < D; ++o) dy[o] = 0.f;
    store10(out + n * D, dy);
    return;
  }
  const int lane = tid & 63;
  // (wave-uniform by construction; said so to the compiler: scalar loads, scalar branches in the walk)
  const int slice = __builtin_amdgcn_readfirstlane((tn ? tile * (tn >> 6) : C.tile_slice[tile]) + (tid >> 6));
  const int srow0 = C.slice_off[slice];
  const int nslots = C.slice_deg[slice];
  const uint32_t* si = slot + (int64_t)srow0 * 64 + lane;
  // all slot dwords of the node are requested at once (clamped index: unconditional loads), ahead of the own-side projections
  uint32_t sw[LIN_CHUNK];
#pragma unroll
  for (int i = 0; i < LIN_CHUNK; ++i) sw[i] = 0u;
  if (nslots > 0) {
#pragma unroll
    for (int i = 0; i < LIN_CHUNK; ++i) sw[i] = si[(int64_t)min(i, nslots - 1) * 64];
  }
  const float4* rp = reinterpret_cast<const float4*>(rec + n * LIN_REC);
  v2f dPt[5], dPf[5], dS_to[5], dS_fr[5];
#pragma unroll
  for (int p = 0; p < 5; ++p) dPt[p] = dPf[p] = dS_to[p] = dS_fr[p] = splat(0.f);
  PHASE();
  mv2<D>(T + L::T_W1I_TO, dx, dPt);
  PHASE();
  mv2<D>(T + L::T_W1I_FR, dx, dPf);
  bool neu = false;
  if constexpr (NEU) {   // a Neumann row: its (only) bit field is Phi_neumann's -- own projection and neighbour column of Phi_neumann
    neu = fl & FLAG_NEUMANN;
    v2f dPn[5];
#pragma unroll
    for (int p = 0; p < 5; ++p) dPn[p] = splat(0.f);
    PHASE();
    mv2<D>(W + tnofs + L::N_W1I, dx, dPn);
#pragma unroll
    for (int p = 0; p < 5; ++p) dPf[p] = neu ? dPn[p] : dPf[p];
  }
  for (int r0 = 0; r0 < nslots; r0 += LIN_CHUNK) {
#pragma unroll
    for (int i = 0; i < LIN_CHUNK; ++i) {
      if (r0 + i < nslots) {   // wave-uniform
        const uint32_t w = sw[i];
        const float4* q = reinterpret_cast<const float4*>(lds + (int)(w & 1023u) * RS);
        const float4 v0 = q[0], v1 = q[1], v2 = q[2], v3 = q[3], v4 = q[4];
        float d[20] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w, v2.x, v2.y,
                       v2.z, v2.w, v3.x, v3.y, v3.z, v3.w, v4.x, v4.y, v4.z, v4.w};
        if constexpr (NEU) {
          const float4 v5 = q[5], v6 = q[6];
          const float2 v7 = reinterpret_cast<const float2*>(q + 7)[0];
          const float e[D] = {v5.x, v5.y, v5.z, v5.w, v6.x, v6.y, v6.z, v6.w, v7.x, v7.y};
#pragma unroll
          for (int o = 0; o < D; ++o) d[D + o] = neu ? e[o] : d[D + o];
        }
#pragma unroll
        for (int p = 0; p < 5; ++p) {
          const v2f a = (v2f){d[2 * p], d[2 * p + 1]} + dPt[p];
          const v2f b = (v2f){d[10 + 2 * p], d[11 + 2 * p]} + dPf[p];
          // (v_bfe_i32: the mask bit as 0 / ~0, and-ed into the addend)
          const int m0 = __builtin_amdgcn_sbfe(w, 10 + 2 * p, 1), m1 = __builtin_amdgcn_sbfe(w, 11 + 2 * p, 1);
          const int m2 = __builtin_amdgcn_sbfe(w, 20 + 2 * p, 1), m3 = __builtin_amdgcn_sbfe(w, 21 + 2 * p, 1);
          dS_to[p] += (v2f){__int_as_float(__float_as_int(a.x) & m0), __int_as_float(__float_as_int(a.y) & m1)};
          dS_fr[p] += (v2f){__int_as_float(__float_as_int(b.x) & m2), __int_as_float(__float_as_int(b.y) & m3)};
        }
      }
    }
    if (r0 + LIN_CHUNK < nslots) {   // (rare: a slice with more than LIN_CHUNK slot rows)
#pragma unroll
      for (int i = 0; i < LIN_CHUNK; ++i) sw[i] = si[(int64_t)min(r0 + LIN_CHUNK + i, nslots - 1) * 64];
    }
  }
  // ---- tangent of the gate, the update MLP and LayerNorm
  // the node record and v's own row are not needed during the walk: read them here instead of holding 34 VGPRs across it (the
  // record requested before the walk took 127 VGPRs, four waves per SIMD; removed)
  PHASE();
  const float4 r0 = rp[0], r1 = rp[1], r2 = rp[2], r3 = rp[3], r4 = rp[4], r5 = rp[5];
  load10(tv + n * D, dx);
  if constexpr (NEU) {
    if (neu) {   // dS_fr holds dS_n
      const float* TN = W + tnofs;
      const unsigned hm = __float_as_uint(r0.w);
      v2f dq[5], dy2[5];
#pragma unroll
      for (int p = 0; p < 5; ++p) dq[p] = dy2[p] = splat(0.f);
      PHASE();
      mv2<D>(TN + L::N_N1H, dx, dq);
      PHASE();
      mv2<D>(TN + L::N_GN, reinterpret_cast<const float*>(dS_fr), dq);
#pragma unroll
      for (int p = 0; p < 5; ++p)
        dq[p] = (v2f){(hm >> (2 * p)) & 1u ? dq[p].x : 0.f, (hm >> (2 * p + 1)) & 1u ? dq[p].y : 0.f};
      PHASE();
      mv2<D>(TN + L::N_N2, reinterpret_cast<const float*>(dq), dy2);
      const float* dyn = reinterpret_cast<const float*>(dy2);
      const float yh[D] = {r3.z, r3.w, r4.x, r4.y, r4.z, r4.w, r5.x, r5.y, r5.z, r5.w};
      float dm = 0.f, yd = 0.f;
#pragma unroll
      for (int o = 0; o < D; ++o) {
        dm += dyn[o];
        yd = fmaf(yh[o], dyn[o], yd);
      }
      dm *= (1.f / D);
      yd *= (1.f / D);
#pragma unroll
      for (int o = 0; o < D; ++o) dy[o] = W[L::LN_G + o] * r0.z * (dyn[o] - dm - yh[o] * yd);
      store10(out + n * D, dy);
      return;
    }
  }
  const float* Wf = W + lofs + L::L_FOLD;
  const float* Wa = W + L::AL_W;
  const float* dsto = reinterpret_cast<const float*>(dS_to);
  const float* dsfr = reinterpret_cast<const float*>(dS_fr);
  PHASE();
  float dal = 0.f;
#pragma unroll
  for (int k = 0; k < D; ++k) dal = fmaf(Wa[k], dx[k], dal);
#pragma unroll
  for (int k = 0; k < D; ++k) dal = fmaf(Wf[L::F_ATO + k], dsto[k], dal);
#pragma unroll
  for (int k = 0; k < D; ++k) dal = fmaf(Wf[L::F_AFR + k], dsfr[k], dal);
  const float al = r0.x;
  dal *= r0.y;
  const unsigned hm = __float_as_uint(r0.w);
  v2f dq[5], dupd[5];
#pragma unroll
  for (int p = 0; p < 5; ++p) dq[p] = dupd[p] = splat(0.f);
  PHASE();
  mv2<D>(T + L::T_U1H, dx, dq);
  PHASE();
  mv2<D>(T + L::T_GTO, dsto, dq);
  PHASE();
  mv2<D>(T + L::T_GFR, dsfr, dq);
#pragma unroll
  for (int p = 0; p < 5; ++p)
    dq[p] = (v2f){(hm >> (2 * p)) & 1u ? dq[p].x : 0.f, (hm >> (2 * p + 1)) & 1u ? dq[p].y : 0.f};
  PHASE();
  mv2<D>(T + L::T_U2, reinterpret_cast<const float*>(dq), dupd);
  const float* du = reinterpret_cast<const float*>(dupd);
  const float u[D] = {r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w, r3.x, r3.y};
  const float yh[D] = {r3.z, r3.w, r4.x, r4.y, r4.z, r4.w, r5.x, r5.y, r5.z, r5.w};
  float dm = 0.f, yd = 0.f;
#pragma unroll
  for (int o = 0; o < D; ++o) {
    dy[o] = dx[o] + dal * u[o] + al * du[o];
    dm += dy[o];
    yd = fmaf(yh[o], dy[o], yd);
  }
  dm *= (1.f / D);
  yd *= (1.f / D);
  const float rs = r0.z;
#pragma unroll
  for (int o = 0; o < D; ++o) dy[o] = W[L::LN_G + o] * rs * (dy[o] - dm - yh[o] * yd);
  store10(out + n * D, dy);
}

// ------------------------------------------------------------------------------------------------------------------
// Transposed product: out = J_f(h)^T w from the same stored linearisation (dirichlet plans)
// ------------------------------------------------------------------------------------------------------------------
// r[k] += sum_o WT[k][o] g[o], k < K: the transposed product on the [in k][out o] section, o pairs packed, one horizontal add per k
template <int K>
__device__ __forceinline__ void mvT(const float* __restrict__ WT, const float* g, float* r) {
  const v2f* w = reinterpret_cast<const v2f*>(WT);
  const v2f gp[5] = {(v2f){g[0], g[1]}, (v2f){g[2], g[3]}, (v2f){g[4], g[5]}, (v2f){g[6], g[7]}, (v2f){g[8], g[9]}};
#pragma unroll
  for (int k = 0; k < K; ++k) {
    if (k > 0 && k % MV2_CH == 0) PHASE();
    v2f a = w[k * 5] * gp[0];
#pragma unroll
    for (int p = 1; p < 5; ++p) a = __builtin_elementwise_fma(w[k * 5 + p], gp[p], a);
    r[k] += a.x + a.y;
  }
}

// Node-local backward of one non-Dirichlet row: the transpose of k_jvp_lin's tail (LayerNorm', update MLP, gate) for the cotangent
// wv of the row's output.  c = [c_to | c_fr] = cotangents of dS_to, dS_fr; dx = the direct term (cotangent of the row's own v).
template <int P>
__device__ __forceinline__ void lin_node_back(const float* __restrict__ W, const float* __restrict__ T, int lofs, const float* wv,
                                              const float* __restrict__ recp, float* c, float* dx) {
  using L = WLayout<P>;
  const float4* rp = reinterpret_cast<const float4*>(recp);
  const float4 r0 = rp[0], r1 = rp[1], r2 = rp[2], r3 = rp[3], r4 = rp[4], r5 = rp[5];
  const float u[D] = {r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w, r3.x, r3.y};
  const float yh[D] = {r3.z, r3.w, r4.x, r4.y, r4.z, r4.w, r5.x, r5.y, r5.z, r5.w};
  const float al = r0.x, rs = r0.z;
  const unsigned hm = __float_as_uint(r0.w);
  // LN' = diag(g) rs (I - 1 1^T / D - yh yh^T / D): its transpose applied to w
  float a[D], ma = 0.f, my = 0.f;
#pragma unroll
  for (int o = 0; o < D; ++o) {
    a[o] = W[L::LN_G + o] * rs * wv[o];
    ma += a[o];
    my = fmaf(yh[o], a[o], my);
  }
  ma *= (1.f / D);
  my *= (1.f / D);
  float dalb = 0.f, dyb[D], dub[D];
#pragma unroll
  for (int o = 0; o < D; ++o) {
    dyb[o] = a[o] - ma - yh[o] * my;   // dy = dx + dal u + al du
    dalb = fmaf(u[o], dyb[o], dalb);
    dub[o] = al * dyb[o];
  }
  // du = U2 (hm . dq),  dq = U1h dx + G_to dS_to + G_fr dS_fr
  float dqb[D];
#pragma unroll
  for (int k = 0; k < D; ++k) dqb[k] = 0.f;
  PHASE();
  mvT<D>(T + L::T_U2, dub, dqb);
#pragma unroll
  for (int k = 0; k < D; ++k) dqb[k] = (hm >> k) & 1u ? dqb[k] : 0.f;
  // dal = alpha (1 - alpha) (w_a . dx + a_to . dS_to + a_fr . dS_fr)
  const float g = r0.y * dalb;
  const float* Wf = W + lofs + L::L_FOLD;
  const float* Wa = W + L::AL_W;
  PHASE();
#pragma unroll
  for (int k = 0; k < D; ++k) {
    c[k] = g * Wf[L::F_ATO + k];
    c[D + k] = g * Wf[L::F_AFR + k];
  }
  PHASE();
  mvT<D>(T + L::T_GTO, dqb, c);
  PHASE();
  mvT<D>(T + L::T_GFR, dqb, c + D);
  if (dx) {
    PHASE();
#pragma unroll
    for (int k = 0; k < D; ++k) dx[k] = fmaf(g, Wa[k], dyb[k]);
    PHASE();
    mvT<D>(T + L::T_U1H, dqb, dx);
  }
}

// The same for a Neumann row (Neumann rows stored): the transpose of LN'( N2 (hm . (N1h v + G_n dS_n)) ).  c = [0 | c_neu], the
// cotangent of dS_n in the Phi_from half (the row has no Phi_to / Phi_from sums); dx = N1h^T dq.
template <int P>
__device__ __forceinline__ void lin_node_back_neu(const float* __restrict__ W, const float* __restrict__ TN, const float* wv,
                                                  const float* __restrict__ recp, float* c, float* dx) {
  using L = WLayout<P>;
  const float4* rp = reinterpret_cast<const float4*>(recp);
  const float4 r0 = rp[0], r3 = rp[3], r4 = rp[4], r5 = rp[5];
  const float yh[D] = {r3.z, r3.w, r4.x, r4.y, r4.z, r4.w, r5.x, r5.y, r5.z, r5.w};
  const float rs = r0.z;
  const unsigned hm = __float_as_uint(r0.w);
  float a[D], ma = 0.f, my = 0.f;
#pragma unroll
  for (int o = 0; o < D; ++o) {
    a[o] = W[L::LN_G + o] * rs * wv[o];
    ma += a[o];
    my = fmaf(yh[o], a[o], my);
  }
  ma *= (1.f / D);
  my *= (1.f / D);
  float dyb[D], dqb[D];
#pragma unroll
  for (int o = 0; o < D; ++o) {
    dyb[o] = a[o] - ma - yh[o] * my;
    dqb[o] = 0.f;
  }
  PHASE();
  mvT<D>(TN + L::N_N2, dyb, dqb);
#pragma unroll
  for (int k = 0; k < D; ++k) dqb[k] = (hm >> k) & 1u ? dqb[k] : 0.f;
#pragma unroll
  for (int k = 0; k < 2 * D; ++k) c[k] = 0.f;
  PHASE();
  mvT<D>(TN + L::N_GN, dqb, c + D);
  if (dx) {
#pragma unroll
    for (int k = 0; k < D; ++k) dx[k] = 0.f;
    PHASE();
    mvT<D>(TN + L::N_N1H, dqb, dx);
  }
}

// One launch per product.  Stage 1: [c_to | c_fr] of every tile and halo row -> 80-byte LDS rows (the own row by its lane, which
// keeps its direct term; halo rows over all threads).  Stage 2, node u: own edges through the counts of its own mask bits (a node's
// cotangent of dS is the same on all its slots), neighbour edges through the transposed slot dwords (tslot: the LDS row of the
// neighbour n | n's masks of the pair's slot in n's ELL row): gathered from u's side, fixed order, no atomics.
//   out[u] = dx[u] + W1i_to^T (cnt_to[u] . c_to[u]) + W1i_fr^T (cnt_fr[u] . c_fr[u])
//          + W1j_to^T sum_n m_to(n; u -> n) . c_to[n] + W1j_fr^T sum_n m_fr(n; n -> u) . c_fr[n]
// One tile of the product (k_vjp_lin: dirichlet plans; k_vjp_lin_mixed: mixed plans with the Neumann rows stored).  NEU: a tile with a
// Neumann row among its own and halo rows (a tile without Neumann nodes of its own can have one in its halo).  A Neumann row n has c[n] = [0 | c_neu[n]]; a slot of u whose partner is a
// Neumann row (bit 30 of the transposed slot dword) adds its masked c_neu to a third sum, and
//   out[u] += W1j_neu^T sum_{Neumann n -> u} m_neu(n's OUT slot of the pair) . c_neu[n];  a Neumann u's own side is W1i_neu^T (cnt . c_neu[u])
template <int P, bool NEU>
__device__ __forceinline__ void vjp_lin_tile(const int tile, float* __restrict__ lds, const TileCtx& C, const float* __restrict__ W,
                                             int lofs, int tofs, const uint32_t* __restrict__ slot,
                                             const uint32_t* __restrict__ tslot, const float* __restrict__ rec,
                                             const float* __restrict__ tw, float* __restrict__ out, int tnofs) {
  using L = WLayout<P>;
  constexpr int RS = 20;
  const int tid = threadIdx.x;
  const int tn = C.tile_nodes;
  const int32_t t0 = tn ? tile * tn : C.tile_ptr[tile];
  const int n_t = tn ? min(tn, C.n_nodes - t0) : C.tile_ptr[tile + 1] - t0;
  const int n_h = C.halo_cnt[tile];
  const int32_t* hl = C.halo + (int64_t)tile * HALO_CAP;
  const float* T = W + tofs;
  // ---- stage 1
  float dx[D];
#pragma unroll
  for (int o = 0; o < D; ++o) dx[o] = 0.f;
  for (int row = tid; row < n_t + n_h; row += TILE_THREADS) {
    const int64_t node = row < n_t ? (int64_t)(t0 + row) : (int64_t)hl[row - n_t];
    float c[2 * D];
#pragma unroll
    for (int o = 0; o < 2 * D; ++o) c[o] = 0.f;
    const uint8_t fl = C.flags_p[node];
    if constexpr (NEU) {
      // (one inlined copy of each node-local backward: a halo row's direct term is computed and dropped)
      if (!(fl & FLAG_DIRICHLET)) {   // (Dirichlet wins, as in the tile kernels)
        float wv[D], dn[D];
        load10(tw + node * D, wv);
        if (fl & FLAG_NEUMANN) lin_node_back_neu<P>(W, W + tnofs, wv, rec + node * LIN_REC, c, dn);
        else lin_node_back<P>(W, T, lofs, wv, rec + node * LIN_REC, c, dn);
        if (row < n_t) {
#pragma unroll
          for (int o = 0; o < D; ++o) dx[o] = dn[o];
        }
      }
    } else if (!(fl & FLAG_DIRICHLET)) {   // a Dirichlet row is a copy of H_init: no cotangent flows through it
      float wv[D];
      load10(tw + node * D, wv);
      if (row < n_t) lin_node_back<P>(W, T, lofs, wv, rec + node * LIN_REC, c, dx);
      else lin_node_back<P>(W, T, lofs, wv, rec + node * LIN_REC, c, nullptr);
    }
    float4* q = reinterpret_cast<float4*>(lds + row * RS);
#pragma unroll
    for (int i = 0; i < 5; ++i) q[i] = make_float4(c[4 * i], c[4 * i + 1], c[4 * i + 2], c[4 * i + 3]);
  }
  __syncthreads();
  if (tid >= n_t) return;
  const int64_t n = (int64_t)t0 + tid;
  const int lane = tid & 63;
  const int slice = __builtin_amdgcn_readfirstlane((tn ? tile * (tn >> 6) : C.tile_slice[tile]) + (tid >> 6));
  const int srow0 = C.slice_off[slice];
  const int nslots = C.slice_deg[slice];
  const uint32_t* si = slot + (int64_t)srow0 * 64 + lane;
  const uint32_t* ti = tslot + (int64_t)srow0 * 64 + lane;
  // own mask bits counted in 4-bit fields, one chunk at a time: nib[j] sums bits 10 + j + 4 i (i < 5) of the node's slot dwords
  const bool own = !(C.flags_p[n] & FLAG_DIRICHLET);   // (a Dirichlet row's own slot dwords are not written by the build)
  unsigned cnt_lo[5] = {0u, 0u, 0u, 0u, 0u}, cnt_hi[5] = {0u, 0u, 0u, 0u, 0u};   // two 16-bit counts per word: bits 10 .. 19 | 20 .. 29
  v2f at[5], af[5], an[NEU ? 5 : 1];
#pragma unroll
  for (int p = 0; p < 5; ++p) at[p] = af[p] = splat(0.f);
#pragma unroll
  for (int p = 0; p < (NEU ? 5 : 1); ++p) an[p] = splat(0.f);
  for (int r0 = 0; r0 < nslots; r0 += LIN_CHUNK) {
    uint32_t sw[LIN_CHUNK], xw[LIN_CHUNK];
#pragma unroll
    for (int i = 0; i < LIN_CHUNK; ++i) {   // clamped index: unconditional loads
      const int64_t r = min(r0 + i, nslots - 1);
      xw[i] = ti[r * 64];
      sw[i] = own ? si[r * 64] : 0u;
    }
    unsigned nib[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < LIN_CHUNK; ++i) {
      if (r0 + i < nslots) {   // wave-uniform
        const uint32_t w = xw[i];
        const float4* q = reinterpret_cast<const float4*>(lds + (int)(w & 1023u) * RS);
        const float4 v0 = q[0], v1 = q[1], v2 = q[2], v3 = q[3], v4 = q[4];
        const float d[20] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w, v2.x, v2.y,
                             v2.z, v2.w, v3.x, v3.y, v3.z, v3.w, v4.x, v4.y, v4.z, v4.w};
#pragma unroll
        for (int p = 0; p < 5; ++p) {
          const int m0 = __builtin_amdgcn_sbfe(w, 10 + 2 * p, 1), m1 = __builtin_amdgcn_sbfe(w, 11 + 2 * p, 1);
          const int m2 = __builtin_amdgcn_sbfe(w, 20 + 2 * p, 1), m3 = __builtin_amdgcn_sbfe(w, 21 + 2 * p, 1);
          at[p] += (v2f){__int_as_float(__float_as_int(d[2 * p]) & m0), __int_as_float(__float_as_int(d[2 * p + 1]) & m1)};
          if constexpr (NEU) {   // partner is a Neumann row: its Phi_from field holds Phi_neumann's masks, its c row c_neu
            const int nm = __builtin_amdgcn_sbfe(w, 30, 1);
            af[p] += (v2f){__int_as_float(__float_as_int(d[10 + 2 * p]) & m2 & ~nm), __int_as_float(__float_as_int(d[11 + 2 * p]) & m3 & ~nm)};
            an[p] += (v2f){__int_as_float(__float_as_int(d[10 + 2 * p]) & m2 & nm), __int_as_float(__float_as_int(d[11 + 2 * p]) & m3 & nm)};
          } else {
            af[p] += (v2f){__int_as_float(__float_as_int(d[10 + 2 * p]) & m2), __int_as_float(__float_as_int(d[11 + 2 * p]) & m3)};
          }
        }
        const uint32_t s = sw[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) nib[j] += (s >> (10 + j)) & 0x11111u;
      }
    }
    // flush (at most LIN_CHUNK < 16 per nibble): bit 10 + b sits in nib[b & 3], nibble b >> 2
#pragma unroll
    for (int b = 0; b < 2 * D; ++b) {
      const unsigned v = (nib[b & 3] >> (4 * (b >> 2))) & 15u;
      if (b < D) cnt_lo[b >> 1] += v << (16 * (b & 1));
      else cnt_hi[(b - D) >> 1] += v << (16 * (b & 1));
    }
  }
  // ---- out = dx + W1i^T (cnt . c_own) + W1j^T (gathered sums)
  const float4* q = reinterpret_cast<const float4*>(lds + tid * RS);
  const float4 v0 = q[0], v1 = q[1], v2 = q[2], v3 = q[3], v4 = q[4];
  const float co[20] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w, v2.x, v2.y,
                        v2.z, v2.w, v3.x, v3.y, v3.z, v3.w, v4.x, v4.y, v4.z, v4.w};
  float gt[D], gf[D];
#pragma unroll
  for (int o = 0; o < D; ++o) {
    gt[o] = (float)((cnt_lo[o >> 1] >> (16 * (o & 1))) & 0xFFFFu) * co[o];
    gf[o] = (float)((cnt_hi[o >> 1] >> (16 * (o & 1))) & 0xFFFFu) * co[D + o];
  }
  if (NEU && (C.flags_p[n] & (FLAG_DIRICHLET | FLAG_NEUMANN)) == FLAG_NEUMANN) {   // (gt = 0: the row's Phi_to bits and c_to are 0)
    PHASE();
    mvT<D>(W + tnofs + L::N_W1I, gf, dx);
  } else {
    PHASE();
    mvT<D>(T + L::T_W1I_TO, gt, dx);
    PHASE();
    mvT<D>(T + L::T_W1I_FR, gf, dx);
  }
  PHASE();
  mvT<D>(T + L::T_W1J_TO, reinterpret_cast<const float*>(at), dx);
  PHASE();
  mvT<D>(T + L::T_W1J_FR, reinterpret_cast<const float*>(af), dx);
  if constexpr (NEU) {
    PHASE();
    mvT<D>(W + tnofs + L::N_W1J, reinterpret_cast<const float*>(an), dx);
  }
  store10(out + n * D, dx);
}

template <int P>
__global__ __launch_bounds__(TILE_THREADS) void k_vjp_lin(int n_tiles, int chunk, const TileCtx C, const float* __restrict__ W,
                                                          int lofs, int tofs, const uint32_t* __restrict__ slot,
                                                          const uint32_t* __restrict__ tslot, const float* __restrict__ rec,
                                                          const float* __restrict__ tw, float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tile = xcd_tile_slot(chunk);
  if (tile >= n_tiles) return;
  vjp_lin_tile<P, false>(tile, lds, C, W, lofs, tofs, slot, tslot, rec, tw, out, 0);
}

// Mixed plans, Neumann rows stored: ONE launch over the handle's tile list (chunk * 8 entries; -1 = none).  An entry with LIN_VNEU set
// is a tile with a Neumann row among its own and halo rows and runs the Neumann form, every other tile the plain form -- a
// workgroup-uniform branch between the two inlined bodies.  The list puts the (few, longer-running) Neumann tiles on the first
// workgroups of the grid, round-robin over the eight XCDs, so that they start first and the plain tiles fill in behind them: as a
// launch of their own they took as long as a single tile takes (21 us for 80 tiles at 582k nodes) behind 43 us of plain tiles.
#define LIN_VNEU 0x40000000
template <int P>
__global__ __launch_bounds__(TILE_THREADS) void k_vjp_lin_mixed(int chunk, const int32_t* __restrict__ tile_list, const TileCtx C,
                                                                const float* __restrict__ W, int lofs, int tofs, int tnofs,
                                                                const uint32_t* __restrict__ slot, const uint32_t* __restrict__ tslot,
                                                                const float* __restrict__ rec, const float* __restrict__ tw,
                                                                float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int32_t e = tile_list[xcd_tile_slot(chunk)];
  if (e < 0) return;
  if (e & LIN_VNEU) vjp_lin_tile<P, true>(e & (LIN_VNEU - 1), lds, C, W, lofs, tofs, slot, tslot, rec, tw, out, tnofs);
  else vjp_lin_tile<P, false>(e, lds, C, W, lofs, tofs, slot, tslot, rec, tw, out, tnofs);
}

// Batched transposed product (solver.hip psignn_broyden_solve_adjoint_lin_batch): ONE launch computes out_m = J_m^T w_m for every
// mesh m of a shard.  The tile entries of all meshes form one slot list (mesh m owns slots [slot_base[m], slot_base[m] + n_slots[m]):
// its tiles in order for a dirichlet handle, its own tile list -- chunk * 8 entries, -1 = none, LIN_VNEU = the Neumann form -- for a
// mixed handle with the Neumann rows stored); a workgroup looks its slot's mesh up, loads that mesh's plan context, linearisation
// arrays and vectors from its descriptor and runs the same tile body as k_vjp_lin / k_vjp_lin_mixed: a tile's rows depend on nothing
// but the tile, so every mesh's product has the bits of its own launch.  A mesh whose stop test has fired is skipped tile by tile.
template <int P>
__global__ __launch_bounds__(TILE_THREADS) void k_vjp_lin_batch(const LinBatchDesc* __restrict__ descs, int n_mesh, int n_slots, int chunk,
                                                                int off_done, const float* __restrict__ W, int lofs, int tofs, int tnofs) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int slot = xcd_tile_slot(chunk);
  if (slot >= n_slots) return;
  int m = 0;
  while (m + 1 < n_mesh && descs[m + 1].slot_base <= slot) ++m;   // wave-uniform scalar walk (a shard has few meshes)
  const LinBatchDesc& d = descs[m];
  if (d.st[off_done]) return;
  int32_t e = slot - d.slot_base;
  if constexpr (P == 3) {
    e = d.vlist[e];
    if (e < 0) return;
    if (e & LIN_VNEU) {
      vjp_lin_tile<P, true>(e & (LIN_VNEU - 1), lds, *d.ctx, W, lofs, tofs, d.slot, d.tslot, d.rec, d.w, d.out, tnofs);
      return;
    }
  }
  vjp_lin_tile<P, false>(e, lds, *d.ctx, W, lofs, tofs, d.slot, d.tslot, d.rec, d.w, d.out, tnofs);
}

// Reverse slot map, once per handle, matched per edge DIRECTION (merge_slots in tiles.hip may pair a node's slots differently on the
// two sides: with u -> n twice and n -> u once, mirrored, u's row is [OUT-only, MERGED] and n's [IN-only, IN-only, OUT-only]):
//   u's slot s carries OUT (edge u -> n), the k-th such slot of u towards n  <->  the k-th IN-carrying slot of n towards u:
//     rev[s].x = its index, whose bits 10..19 are n's Phi_to masks of that edge
//   u's slot s carries IN  (edge n -> u), the k-th such slot of u towards n  <->  the k-th OUT-carrying slot of n towards u:
//     rev[s].y = its index, whose bits 20..29 are n's Phi_from masks of that edge
// (both lists are in canonical edge order on both sides, so the k-th of one side is the same edge as the k-th of the other).  -1: no
// such direction.  A direction without a partner (a plan this matching does not understand) sets *bad: the product is refused.
// The low 10 bits of tslot[s] get u's LDS row field of the slot (the masks are filled in per build by k_lin_tfill).
__device__ __forceinline__ int32_t lin_tile_of(const int32_t* __restrict__ a, int n, int32_t x) {   // last i with a[i] <= x
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (a[mid] <= x) lo = mid; else hi = mid;
  }
  return lo;
}
// NEU: bit 30 of tslot[s] = the slot's neighbour is a Neumann row (kept by k_lin_tfill)
template <bool NEU = false>
__global__ __launch_bounds__(256) void k_lin_rev(int64_t n_slices, int n_tiles, const TileCtx C, int2* __restrict__ rev,
                                                 uint32_t* __restrict__ tslot, int32_t* __restrict__ bad) {
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t s = gid >> 6;
  if (s >= n_slices) return;
  const int lane = (int)(gid & 63);
  const int tile = lin_tile_of(C.tile_slice, n_tiles, (int32_t)s);
  const int32_t t0 = C.tile_ptr[tile], n_t = C.tile_ptr[tile + 1] - t0;
  const int32_t u = t0 + 64 * (int32_t)(s - C.tile_slice[tile]) + lane;
  const int64_t row0 = C.slice_off[s];
  const int deg = C.slice_deg[s];
  const int32_t* hl = C.halo + (int64_t)tile * HALO_CAP;
  for (int r = 0; r < deg; ++r) {
    const int64_t idx = (row0 + r) * 64 + lane;
    int2 found = make_int2(-1, -1);
    uint32_t li = 0;
    const uint32_t e = u < t0 + n_t ? C.ell[idx].x : ELL_EMPTY;
    if ((e & 0xFFFFu) != ELL_EMPTY) {
      li = e & 0xFFFFu;
      const uint32_t kind = (e >> 16) & 3u;
      int k_out = 0, k_in = 0;   // earlier OUT- / IN-carrying slots of u towards the same neighbour
      for (int r2 = 0; r2 < r; ++r2) {
        const uint32_t e2 = C.ell[(row0 + r2) * 64 + lane].x;
        if ((e2 & 0xFFFFu) != li) continue;
        k_out += (e2 & SLOT_OUT) ? 1 : 0;
        k_in += (e2 & SLOT_IN) ? 1 : 0;
      }
      const int32_t nb = (int32_t)li < n_t ? t0 + (int32_t)li : hl[li - n_t];
      const int tile2 = lin_tile_of(C.tile_ptr, n_tiles, nb);
      const int32_t t02 = C.tile_ptr[tile2], n_t2 = C.tile_ptr[tile2 + 1] - t02;
      const int64_t s2 = C.tile_slice[tile2] + (nb - t02) / 64;
      const int lane2 = (nb - t02) & 63;
      const int32_t* hl2 = C.halo + (int64_t)tile2 * HALO_CAP;
      const int64_t row02 = C.slice_off[s2];
      const bool want_to = kind & 2u, want_fr = kind & 1u;
      for (int r2 = 0; r2 < C.slice_deg[s2]; ++r2) {
        const int64_t idx2 = (row02 + r2) * 64 + lane2;
        const uint32_t e2 = C.ell[idx2].x;
        if ((e2 & 0xFFFFu) == ELL_EMPTY) continue;
        const uint32_t li2 = e2 & 0xFFFFu;
        const int32_t back = (int32_t)li2 < n_t2 ? t02 + (int32_t)li2 : hl2[li2 - n_t2];
        if (back != u) continue;
        if (want_to && found.x < 0 && (e2 & SLOT_IN) && k_out-- == 0) found.x = (int32_t)idx2;
        if (want_fr && found.y < 0 && (e2 & SLOT_OUT) && k_in-- == 0) found.y = (int32_t)idx2;
      }
      if ((want_to && found.x < 0) || (want_fr && found.y < 0)) atomicOr(bad, 1);
      if (NEU && (C.flags_p[nb] & FLAG_NEUMANN)) li |= 1u << 30;
    }
    rev[idx] = found;
    tslot[idx] = li;
  }
}

// Per build: the neighbour's masks of each edge direction next to the LDS row field (bits 10 .. 29, as in the slot dwords)
__global__ __launch_bounds__(256) void k_lin_tfill(int64_t n, const int2* __restrict__ rev, const uint32_t* __restrict__ slot,
                                                   uint32_t* __restrict__ tslot) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int2 r = rev[i];
  tslot[i] = (tslot[i] & 0x400003FFu) | (r.x >= 0 ? slot[r.x] & 0x000FFC00u : 0u) | (r.y >= 0 ? slot[r.y] & 0x3FF00000u : 0u);
}

// ------------------------------------------------------------------------------------------------------------------ host
// flag[tile] = 1: a Neumann row among the tile's own and halo rows (the transposed product's tile groups, once per handle)
__global__ __launch_bounds__(64) void k_lin_vgroup(const TileCtx C, int32_t* __restrict__ flag) {
  const int tile = blockIdx.x;
  const int32_t t0 = C.tile_ptr[tile];
  const int n_t = C.tile_ptr[tile + 1] - t0, n_h = C.halo_cnt[tile];
  const int32_t* hl = C.halo + (int64_t)tile * HALO_CAP;
  bool any = false;
  for (int row = threadIdx.x; row < n_t + n_h; row += 64) {
    const uint8_t fl = C.flags_p[row < n_t ? t0 + row : hl[row - n_t]];
    any |= (fl & (FLAG_DIRICHLET | FLAG_NEUMANN)) == FLAG_NEUMANN;
  }
  if (__ballot(any) != 0ull && threadIdx.x == 0) flag[tile] = 1;
}

extern "C" int psignn_lin_create(psignn_lin_t** out, const psignn_plan_t* p) { return psignn_lin_create_opts(out, p, 0); }

extern "C" int psignn_lin_neumann_stored(const psignn_lin_t* s) { return s ? s->neu : 0; }

extern "C" int psignn_lin_create_opts(psignn_lin_t** out, const psignn_plan_t* p, int neumann_stored) {
  ARG_CHECK(out && p, "NULL argument");
  ARG_CHECK(neumann_stored == 0 || neumann_stored == 1, "neumann_stored is 0 or 1");
  ARG_CHECK(p->tiled, "linearised JVP: tiled plans (other plans use psignn_f_jvp)");
  ARG_CHECK(p->max_rows <= 1024, "tile + halo rows exceed the 10-bit row field of the stored slots");
  psignn_lin* s = new psignn_lin();
  s->plan = p;
  s->neu = p->mixed && neumann_stored;
  const size_t b_slot = (size_t)(p->ell_rows + 1) * 64 * 4, b_rec = (size_t)p->N * LIN_REC * 4;
  const size_t b_state = s->neu ? (size_t)cdiv(p->n_tiles, 8) * 8 * 4 : p->mixed ? (size_t)p->N * (D + 3 + 2) * 4 : 0;
  bool ok = hipMalloc((void**)&s->slot, b_slot) == hipSuccess && hipMalloc((void**)&s->rec, b_rec) == hipSuccess;
  if (ok && s->neu) {
    // tile list of the transposed product (k_vjp_lin_mixed): per-tile flags on the device, arranged on the host, once per handle
    const size_t nt = (size_t)p->n_tiles, chunk = (size_t)cdiv((int64_t)nt, 8), nl = chunk * 8;
    ok = hipMalloc((void**)&s->vlist, (nl > nt ? nl : nt) * 4 + 4) == hipSuccess;
    if (ok && nt > 0) {
      int32_t* fl = (int32_t*)malloc(nt * 4);
      int32_t* ord = (int32_t*)malloc(nl * 4);
      hipError_t e = fl && ord ? hipMemset(s->vlist, 0, nt * 4) : hipErrorOutOfMemory;
      if (e == hipSuccess) {
        k_lin_vgroup<<<(unsigned)nt, 64>>>(p->h_ctx, s->vlist);
        e = hipMemcpy(fl, s->vlist, nt * 4, hipMemcpyDeviceToHost);
      }
      if (e == hipSuccess) {
        // workgroup b of the grid reads entry xcd_slot(b, chunk): the j-th Neumann tile goes where workgroup j reads, the
        // plain tiles fill the other entries in ascending order (neighbouring tiles stay on one XCD, as in the other tile kernels)
        for (size_t i = 0; i < nl; ++i) ord[i] = -1;
        size_t j = 0;
        for (size_t t = 0; t < nt; ++t)
          if (fl[t]) {
            ord[xcd_slot((unsigned)j, (int)chunk)] = (int32_t)t | LIN_VNEU;
            ++j;
          }
        s->n_vplain = (int)(nt - j);
        size_t pos = 0;
        for (size_t t = 0; t < nt; ++t)
          if (!fl[t]) {
            while (ord[pos] != -1) ++pos;
            ord[pos] = (int32_t)t;
          }
        e = hipMemcpy(s->vlist, ord, nl * 4, hipMemcpyHostToDevice);
      }
      free(fl);
      free(ord);
      if (e != hipSuccess) {
        (void)hipGetLastError();
        psignn_lin_destroy(s);
        psignn_set_error("psignn_lin_create_opts: tile list of the transposed product -> %s", hipGetErrorString(e));
        return PSIGNN_EHIP;
      }
    }
  } else if (ok && p->mixed)
    ok = hipMalloc((void**)&s->h, (size_t)p->N * D * 4) == hipSuccess && hipMalloc((void**)&s->prb, (size_t)p->N * 3 * 4) == hipSuccess &&
         hipMalloc((void**)&s->nrm, (size_t)p->N * 2 * 4) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    psignn_lin_destroy(s);
    psignn_set_error("psignn_lin_create: out of device memory (%zu bytes)", b_slot + b_rec + b_state);
    return PSIGNN_ENOMEM;
  }
  s->bytes = b_slot + b_rec + b_state;
  *out = s;
  return PSIGNN_OK;
}

extern "C" void psignn_lin_destroy(psignn_lin_t* s) {
  if (!s) return;
  for (void* q : {(void*)s->slot, (void*)s->rec, (void*)s->h, (void*)s->prb, (void*)s->nrm, (void*)s->rev, (void*)s->tslot, (void*)s->vlist})
    if (q) (void)hipFree(q);
  delete s;
}

extern "C" size_t psignn_lin_bytes(const psignn_lin_t* s) { return s ? s->bytes + s->tbytes : 0; }

// h, prb (and, mixed plans, the unit normals) in PLAN order; dirichlet: single-layer block; mixed: any depth (the iterated layer is
// the last one, as in psignn_f_jvp)
extern "C" int psignn_lin_build(psignn_lin_t* s, const float* W, int nl, const float* h, const float* prb, const float* nrm,
                                void* stream) {
  ARG_CHECK(s && W && h && prb, "NULL argument");
  const psignn_plan* p = s->plan;
  ARG_CHECK(p->mixed ? nl >= 1 : nl == 1, "linearised JVP: single-layer blocks (mixed plans: the last layer)");
  ARG_CHECK(!p->mixed || nrm, "mixed plan needs unit normals");
  hipStream_t st = (hipStream_t)stream;
  const size_t lds = (size_t)p->max_rows * 20 * 4;
  if (p->mixed) {
    using L = WLayout<3>;
    const int na = (int)p->n_tiles_plain, nb = (int)(p->n_tiles - p->n_tiles_plain);
    if (s->neu) {
      if (nb > 0) {   // the tiles holding Neumann nodes: 144-byte LDS rows, Neumann rows stored
        const int chunk = (int)cdiv(nb, 8);
        // the group's share of the plan by tiles (node counts per group are not kept on the host), normals included (8 N)
        PROF_BYTES(((70 * p->N + 20 * p->Ep) + (int64_t)p->N * LIN_REC * 4 + (int64_t)p->ell_rows * 64 * 4) * nb / p->n_tiles);
        LAUNCH("k_lin_build_neu", st, (k_lin_build<3, true><<<(unsigned)(chunk * 8), TILE_THREADS, (size_t)p->max_rows * LIN_RS_NEU * 4, st>>>(
            nb, chunk, p->tile_order + na, p->h_ctx, W, L::layer(nl - 1), L::tp_layer(nl, true, nl - 1), h, prb, s->slot, s->rec,
            L::tp_neu(nl), nrm)));
      }
    } else {
      HIP_TRY(hipMemcpyAsync(s->h, h, (size_t)p->N * D * 4, hipMemcpyDeviceToDevice, st));
      HIP_TRY(hipMemcpyAsync(s->prb, prb, (size_t)p->N * 3 * 4, hipMemcpyDeviceToDevice, st));
      HIP_TRY(hipMemcpyAsync(s->nrm, nrm, (size_t)p->N * 2 * 4, hipMemcpyDeviceToDevice, st));
    }
    if (na > 0) {
      const int chunk = (int)cdiv(na, 8);
      // (Neumann rows stored: the plain group's share by tiles; otherwise the launch is the handle's only build launch)
      PROF_BYTES(((62 * p->N + 20 * p->Ep) + (int64_t)p->N * LIN_REC * 4 + (int64_t)p->ell_rows * 64 * 4) * (s->neu ? na : p->n_tiles) /
                 p->n_tiles);
      LAUNCH("k_lin_build", st, (k_lin_build<3><<<(unsigned)(chunk * 8), TILE_THREADS, lds, st>>>(
          na, chunk, p->tile_order, p->h_ctx, W, L::layer(nl - 1), L::tp_layer(nl, true, nl - 1), h, prb, s->slot, s->rec)));
    }
  } else {
    using L = WLayout<2>;
    const int chunk = (int)cdiv(p->n_tiles, 8);
    // B_f's reads (h, prb, flags, slot records) + the stored linearisation
    PROF_BYTES((49 * p->N + 20 * p->Ep) + (int64_t)p->N * LIN_REC * 4 + (int64_t)p->ell_rows * 64 * 4);
    LAUNCH("k_lin_build", st, (k_lin_build<2><<<(unsigned)(chunk * 8), TILE_THREADS, lds, st>>>(
        (int)p->n_tiles, chunk, nullptr, p->h_ctx, W, L::layer(0), L::tp_layer(nl, false, 0), h, prb, s->slot, s->rec)));
  }
  HIP_TRY(hipGetLastError());
  s->built = 1;
  s->tfilled = 0;
  return PSIGNN_OK;
}

// v, out in PLAN order: out = J_f(h) v for the h of the last psignn_lin_build
extern "C" int psignn_lin_jvp(const psignn_lin_t* s, const float* W, int nl, const float* v, float* out, void* stream) {
  ARG_CHECK(s && W && v && out, "NULL argument");
  ARG_CHECK(s->built, "psignn_lin_build has not run");
  ARG_CHECK(v != out, "in-place product is not supported");
  const psignn_plan* p = s->plan;
  ARG_CHECK(p->mixed ? nl >= 1 : nl == 1, "linearised JVP: single-layer blocks (mixed plans: the last layer)");
  hipStream_t st = (hipStream_t)stream;
  const size_t lds = (size_t)p->max_rows * 20 * 4;
  if (p->mixed) {
    using L = WLayout<3>;
    const int na = (int)p->n_tiles_plain;
    if (na > 0) {
      const int chunk = (int)cdiv(na, 8);
      PROF_BYTES(((int64_t)p->N * (81 + LIN_REC * 4) + (int64_t)p->ell_rows * 64 * 4) * (s->neu ? na : p->n_tiles) / p->n_tiles);
      LAUNCH("k_jvp_lin", st, (k_jvp_lin<3><<<(unsigned)(chunk * 8), TILE_THREADS, lds, st>>>(
          na, chunk, p->tile_order, p->h_ctx, W, L::layer(nl - 1), L::tp_layer(nl, true, nl - 1), s->slot, s->rec, v, out)));
    }
    const int nb = (int)(p->n_tiles - p->n_tiles_plain);
    if (!s->neu) {
      int rc = psignn_f_tile_jvp_groups(p, W, nl, s->h, s->prb, s->nrm, v, out, 2, st);   // the tiles holding Neumann nodes
      if (rc) return rc;
    } else if (nb > 0) {   // the same stored operator on the tiles holding Neumann nodes (144-byte LDS rows)
      const int chunk = (int)cdiv(nb, 8);
      PROF_BYTES(((int64_t)p->N * (81 + LIN_REC * 4) + (int64_t)p->ell_rows * 64 * 4) * nb / p->n_tiles);   // share by tiles
      LAUNCH("k_jvp_lin_neu", st, (k_jvp_lin<3, true><<<(unsigned)(chunk * 8), TILE_THREADS, (size_t)p->max_rows * LIN_RS_NEU * 4, st>>>(
          nb, chunk, p->tile_order + na, p->h_ctx, W, L::layer(nl - 1), L::tp_layer(nl, true, nl - 1), s->slot, s->rec, v, out,
          L::tp_neu(nl))));
    }
  } else {
    using L = WLayout<2>;
    const int chunk = (int)cdiv(p->n_tiles, 8);
    // v, out (40 N each), flags (N), node records, slot dwords
    PROF_BYTES((int64_t)p->N * (81 + LIN_REC * 4) + (int64_t)p->ell_rows * 64 * 4);
    LAUNCH("k_jvp_lin", st, (k_jvp_lin<2><<<(unsigned)(chunk * 8), TILE_THREADS, lds, st>>>(
        (int)p->n_tiles, chunk, nullptr, p->h_ctx, W, L::layer(0), L::tp_layer(nl, false, 0), s->slot, s->rec, v, out)));
  }
  HIP_TRY(hipGetLastError());
  return PSIGNN_OK;
}

// w, out in PLAN order: out = J_f(h)^T w for the h of the last psignn_lin_build.  Dirichlet plans: k_vjp_lin (one launch; on the first
// call after a build also k_lin_tfill, on the first call of the handle k_lin_rev and the two transposed arrays).  Mixed plans: the
// tiled VJP (psignn_f_tile_vjp, work = the plan workspace) at the state kept by the build; with the Neumann rows stored
// (psignn_lin_create_opts) one k_vjp_lin_mixed launch over the handle's tile list, work ignored.

// The transposed product's lazy work: on the first call of the handle the two transposed arrays and k_lin_rev, on the first call after a
// build k_lin_tfill.  (The batched product runs it per handle in its prologue, never inside the lockstep loop.)
static int lin_vjp_prepare(const psignn_lin* s, hipStream_t st) {
  const psignn_plan* p = s->plan;
  const int64_t n_sl = p->ell_rows * 64;
  if (!s->tslot) {
    const size_t nb = (size_t)(p->ell_rows + 1) * 64, b = nb * 4 + nb * 8 + 4;
    int32_t* bad = nullptr;
    if (hipMalloc((void**)&s->rev, nb * 8 + 4) != hipSuccess || hipMalloc((void**)&s->tslot, nb * 4) != hipSuccess) {
      (void)hipGetLastError();
      if (s->rev) (void)hipFree(s->rev);
      s->rev = nullptr;
      s->tslot = nullptr;
      psignn_set_error("psignn_lin_vjp: out of device memory (%zu bytes)", b);
      return PSIGNN_ENOMEM;
    }
    s->tbytes = b;
    bad = reinterpret_cast<int32_t*>(s->rev + nb);   // one flag word behind the map
    HIP_TRY(hipMemsetAsync(s->rev, 0xFF, nb * 8, st));
    HIP_TRY(hipMemsetAsync(bad, 0, 4, st));
    HIP_TRY(hipMemsetAsync(s->tslot, 0, nb * 4, st));
    if (p->n_slices > 0) {
      if (s->neu)
        LAUNCH("k_lin_rev", st, (k_lin_rev<true><<<(unsigned)cdiv(p->n_slices * 64, 256), 256, 0, st>>>(
            p->n_slices, (int)p->n_tiles, p->h_ctx, s->rev, s->tslot, bad)));
      else
        LAUNCH("k_lin_rev", st, (k_lin_rev<false><<<(unsigned)cdiv(p->n_slices * 64, 256), 256, 0, st>>>(
            p->n_slices, (int)p->n_tiles, p->h_ctx, s->rev, s->tslot, bad)));
    }
    int32_t h_bad = 0;   // (once per handle)
    HIP_TRY(hipMemcpyAsync(&h_bad, bad, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (h_bad) {
      (void)hipFree(s->rev);
      (void)hipFree(s->tslot);
      s->rev = nullptr;
      s->tslot = nullptr;
      s->tbytes = 0;
      psignn_set_error("psignn_lin_vjp: an edge direction of the plan's slots has no partner slot at its neighbour");
      return PSIGNN_EINVAL;
    }
    s->tfilled = 0;
  }
  if (!s->tfilled) {
    if (n_sl > 0)
      LAUNCH("k_lin_tfill", st, (k_lin_tfill<<<(unsigned)cdiv(n_sl, 256), 256, 0, st>>>(n_sl, s->rev, s->slot, s->tslot)));
    s->tfilled = 1;
  }
  return PSIGNN_OK;
}

extern "C" int psignn_lin_vjp(const psignn_lin_t* s, const float* W, int nl, const float* w, float* out, float* work, void* stream) {
  ARG_CHECK(s && W && w && out, "NULL argument");
  ARG_CHECK(s->built, "psignn_lin_build has not run");
  ARG_CHECK(w != out, "in-place product is not supported");
  const psignn_plan* p = s->plan;
  ARG_CHECK(p->mixed ? nl >= 1 : nl == 1, "linearised VJP: single-layer blocks (mixed plans: the last layer)");
  hipStream_t st = (hipStream_t)stream;
  if (p->mixed && !s->neu) {
    ARG_CHECK(work, "mixed plan: the transposed product needs the plan workspace");
    return psignn_f_tile_vjp(p, W, nl, s->h, s->prb, s->nrm, w, out, work, st);
  }
  if (int rc = lin_vjp_prepare(s, st)) return rc;
  const size_t lds = (size_t)p->max_rows * 20 * 4;
  if (s->neu) {   // mixed plan, Neumann rows stored: one launch, the Neumann form on the tiles with a Neumann row among tile + halo
    using L = WLayout<3>;
    const int chunk = (int)cdiv(p->n_tiles, 8);
    if (chunk > 0) {
      // w, out (40 N each), flags, node records, slot and transposed slot dwords
      PROF_BYTES((int64_t)p->N * (81 + LIN_REC * 4) + (int64_t)p->ell_rows * 64 * 8);
      LAUNCH("k_vjp_lin_mixed", st, (k_vjp_lin_mixed<3><<<(unsigned)(chunk * 8), TILE_THREADS, lds, st>>>(
          chunk, s->vlist, p->h_ctx, W, L::layer(nl - 1), L::tp_layer(nl, true, nl - 1), L::tp_neu(nl), s->slot, s->tslot, s->rec, w,
          out)));
    }
    HIP_TRY(hipGetLastError());
    return PSIGNN_OK;
  }
  using L = WLayout<2>;
  const int chunk = (int)cdiv(p->n_tiles, 8);
  // w (tile + halo rows), out (40 N each), flags, node records (tile + halo rows), slot and transposed slot dwords
  PROF_BYTES((int64_t)p->N * (81 + LIN_REC * 4) + (int64_t)p->ell_rows * 64 * 8);
  LAUNCH("k_vjp_lin", st, (k_vjp_lin<2><<<(unsigned)(chunk * 8), TILE_THREADS, lds, st>>>(
      (int)p->n_tiles, chunk, p->h_ctx, W, L::layer(0), L::tp_layer(nl, false, 0), s->slot, s->tslot, s->rec, w, out)));
  HIP_TRY(hipGetLastError());
  return PSIGNN_OK;
}

const psignn_plan* psignn_lin_plan(const psignn_lin_t* s) { return s ? s->plan : nullptr; }

// ---- batched transposed product (solver.hip)
// 1 when the batch product takes this handle for a solver of plan p: made for p, built, dirichlet or mixed with the Neumann rows stored
int psignn_lin_batch_ok(const psignn_lin_t* s, const psignn_plan* p) {
  return s && p && s->plan == p && s->built && (!p->mixed || s->neu) ? 1 : 0;
}

// algorithmic bytes of one transposed product of the handle (as psignn_lin_vjp states them)
int64_t psignn_lin_vjp_bytes(const psignn_lin_t* s) {
  const psignn_plan* p = s->plan;
  return (int64_t)p->N * (81 + LIN_REC * 4) + (int64_t)p->ell_rows * 64 * 8;
}

// The handle's part of its mesh descriptor (d->w, d->out, d->st, d->slot_base are the caller's), after the lazy work of psignn_lin_vjp
int psignn_lin_batch_fill(const psignn_lin_t* s, LinBatchDesc* d, hipStream_t st) {
  ARG_CHECK(s && d && s->built, "psignn_lin_build has not run");
  const psignn_plan* p = s->plan;
  ARG_CHECK(!p->mixed || s->neu, "batched transposed product: mixed handles need the Neumann rows stored");
  if (int rc = lin_vjp_prepare(s, st)) return rc;
  d->ctx = p->d_ctx;
  d->slot = s->slot;
  d->tslot = s->tslot;
  d->rec = s->rec;
  d->vlist = s->neu ? s->vlist : nullptr;
  d->n_slots = s->neu ? (int32_t)cdiv(p->n_tiles, 8) * 8 : (int32_t)p->n_tiles;
  return PSIGNN_OK;
}

// descs: device array of n_mesh descriptors of ONE family; max_rows: largest tile + halo row count over the meshes (LDS size)
int psignn_lin_vjp_batch(const LinBatchDesc* d_descs, int n_mesh, int n_slots, int max_rows, const float* W, int mixed, int off_done,
                         hipStream_t st) {
  const int chunk = (int)cdiv(n_slots, 8);
  if (chunk <= 0) return PSIGNN_OK;
  const size_t lds = (size_t)max_rows * 20 * 4;
  if (mixed) {
    using L = WLayout<3>;
    LAUNCH("k_vjp_lin_batch", st, (k_vjp_lin_batch<3><<<(unsigned)(chunk * 8), TILE_THREADS, lds, st>>>(
        d_descs, n_mesh, n_slots, chunk, off_done, W, L::layer(0), L::tp_layer(1, true, 0), L::tp_neu(1))));
  } else {
    using L = WLayout<2>;
    LAUNCH("k_vjp_lin_batch", st, (k_vjp_lin_batch<2><<<(unsigned)(chunk * 8), TILE_THREADS, lds, st>>>(
        d_descs, n_mesh, n_slots, chunk, off_done, W, L::layer(0), L::tp_layer(1, false, 0), 0)));
  }
  HIP_TRY(hipGetLastError());
  return PSIGNN_OK;
}
