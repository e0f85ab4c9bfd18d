// f_theta on the tiled plan: one workgroup per mesh tile, neighbour projections staged in LDS (gfx950).
//
// Same function as fgnn.hip (reference: dirichlet/psignn/model.py:279-300, mixed/psignn/model.py:216-245),
// different data movement:
//   stage 1  every lane takes one row of the tile + halo (<= 256 + HALO_CAP rows): loads h (tile rows are
//            one coalesced 40 B/lane stream, halo rows a short indexed gather), projects it with the
//            neighbour-side weights W1j_{to,from[,neu]} and parks the 80-byte result row in LDS
//            (byte counts for the default width D = 10: rows are 4 D bytes in memory, 8 D / 12 D in LDS)
//   stage 2  every lane owns one tile node and walks its pair-merged ELL slots (tiles.hip): one coalesced
//            16-byte load {LDS row, IN/OUT, edge_attr} and one LDS row read (5 x ds_read_b128) serve BOTH
//            directions of a neighbour; relu terms are summed in the plan's canonical order (no atomics,
//            bitwise reproducible), then gate / update MLP / LayerNorm / boundary rows.
// The second Phi layer (W2 S + deg b2) is linear and is folded into the consumers' first-layer weights on
// the host (WLayout fold block).  All node tensors are in PLAN order; the solver keeps its state there.
// weight loads of mv2 pinned chunk by chunk (tile_helpers.h; A/B in profiles/r3_ab_mv2.txt: fused step 75.8 -> 73.4 us, plain f unchanged)
#define MV2_LAUNDER 2
#define MV2_CH (100 / PSIGNN_D)   // at most ~100 weights of a block in flight: 10 inputs at D = 10, 6 at 16, the whole 8 x 8 block at 8
#include "tile_helpers.h"
#include "internal.h"
// Occupancy caps were measured and removed (profiles/r2_f_tile_ab_runs.txt): k_f_tile held to 96 VGPRs ran plain f in 59.8 vs
// 58.0 us, the fused instantiations held to 80 VGPRs for a sixth wave 89.6 vs 88.8 us, the batched kernel held to six waves 57.4
// vs 50.7 us at 8 x 50k nodes.

template <bool MIXED>
struct TileRow {
  static constexpr int RS = MIXED ? (3 * D + 3) / 4 * 4 : 2 * D;  // floats per LDS row: [to D | from D] (| neu D | pad to 16 bytes)
};
static_assert(TileRow<false>::RS % 4 == 0 && TileRow<true>::RS % 4 == 0, "LDS rows are read as 16-byte quads");
#if PSIGNN_D == 10
static_assert(TileRow<false>::RS == 20 && TileRow<true>::RS == 32, "LDS rows at D = 10");
#endif
// the largest requests a tiled plan can make fit the 160 KiB of a CU at every width: the plan's row limits are width-free
static_assert((TILE_MAX + HALO_CAP) * TileRow<false>::RS * 4 <= 160 * 1024 && MIXED_ROW_CAP * TileRow<true>::RS * 4 <= 160 * 1024,
              "LDS rows of the f kernel at the plan's row limits");

// LDS row helpers.  A row starts on a 16-byte boundary; a segment of D floats (NPAIR register pairs) at float offset OFF starts on
// one too when OFF is a multiple of 4, else (D = 2 mod 4, second segment) at 8 mod 16.
// [a | b] = 2 D floats from the row's start: NPAIR quads (D = 10: 5 x ds_write_b128)
__device__ __forceinline__ void lds_store_row2(float* __restrict__ rowp, const v2f* a, const v2f* b) {
  float4* q = reinterpret_cast<float4*>(rowp);
  v2f c[2 * NPAIR];
#pragma unroll
  for (int p = 0; p < NPAIR; ++p) {
    c[p] = a[p];
    c[NPAIR + p] = b[p];
  }
#pragma unroll
  for (int i = 0; i < NPAIR; ++i) q[i] = make_float4(c[2 * i].x, c[2 * i].y, c[2 * i + 1].x, c[2 * i + 1].y);
}
// one segment: quads and, when D is not a multiple of 4, one b64 -- at the end of an aligned segment (D = 10: b128, b128, b64),
// at the start of one that begins at 8 mod 16 (b64, b128, b128)
template <int OFF>
__device__ __forceinline__ void lds_store_row(float* __restrict__ rowp, const v2f* t) {
  static_assert(OFF % 4 == 0 || (OFF % 2 == 0 && D % 4 == 2), "segment start");
  if constexpr (OFF % 4 == 0) {
    float4* q = reinterpret_cast<float4*>(rowp + OFF);
#pragma unroll
    for (int i = 0; i < D / 4; ++i) q[i] = make_float4(t[2 * i].x, t[2 * i].y, t[2 * i + 1].x, t[2 * i + 1].y);
    if (D % 4) reinterpret_cast<float2*>(rowp + OFF)[NPAIR - 1] = make_float2(t[NPAIR - 1].x, t[NPAIR - 1].y);
  } else {
    reinterpret_cast<float2*>(rowp + OFF)[0] = make_float2(t[0].x, t[0].y);
    float4* q = reinterpret_cast<float4*>(rowp + OFF + 2);
#pragma unroll
    for (int i = 0; i < D / 4; ++i) q[i] = make_float4(t[2 * i + 1].x, t[2 * i + 1].y, t[2 * i + 2].x, t[2 * i + 2].y);
  }
}

// Stage 1 exists in two forms, chosen per launch (env PSIGNN_STAGE1 = mfma | valu overrides the default):
// matrix cores (v_mfma_f32_16x16x4_f32) or packed VALU.  The matrix-core form is written for D = 10 (K padded to 12, 20 / 30
// outputs in two M-tiles) and exists in that build only: at another width the knob has no effect.
#include <stdlib.h>
#include <string.h>
// Default form: packed VALU everywhere.  A/Bs on one box (1M-node mesh) after the scalar-load phase barriers removed the
// SGPR spills of the VALU form: dirichlet plain f 64.6 us (valu) vs 67.7 us (mfma); fused Broyden step 102 us (valu) vs
// 122-125 us (mfma: it has to re-load x and update for stage 2, which the VALU form gets for free from its stage-1
// registers); mixed plain f 102.9 (valu) vs 102.2 (mfma) in one launch, 81.8 us (valu) once the tiles without Neumann
// nodes run with 80-byte LDS rows (launch_mixed).  Before the barriers the VALU form spilled ~200 SGPRs and lost: 68.2 vs
// 66.3 us.  The MFMA form stays selectable (PSIGNN_STAGE1=mfma) for A/B runs.
constexpr bool MFMA_FORM = D == 10;   // template argument of the launches the knob selects: the VALU form again at another width
static int stage1_mfma(bool fused, bool mixed) {
#if PSIGNN_D != 10
  (void)fused;
  (void)mixed;
  return 0;
#else
  KNOB_INT(forced, [] {
    const char* e = getenv("PSIGNN_STAGE1");
    return !e ? -1 : (strcmp(e, "mfma") == 0 ? 1 : 0);
  }());
  if (forced >= 0) return forced;
  (void)fused;
  (void)mixed;
  return 0;   // the MFMA form is kept for A/B runs (PSIGNN_STAGE1=mfma); see the comment above
#endif
}

// Broyden fusion (solver.hip): the kernel forms x_next = x_cur + update while loading, and its epilogue
// writes x_next, g_new = f(x_next) - x_next, dg = g_new - g_old and the per-wave partials of |g_new|^2, |f|^2
// -- the work of k_xnext and k_resid without their extra passes over the state vectors.
struct FuseArgs {
  const float* upd;   // update vector, plan order
  float* gnew;        // out: g = f(x_next) - x_next  (g of the previous iterate stays in the solver's other g buffer: the
                      // update kernels form dg = g_new - g_old themselves; round 2 read g_old and wrote dg here, +80 MB/step at 1M nodes)
  float* xbuf;        // iterate buffers (stride M)
  const int32_t* st;  // device status block (int32 view)
  int off_done, off_cur, off_nxt;
  int64_t M;
  float* part;
  int npart;
  long long* stamps;  // diagnostics (psignn_prof_tile_stamps): per tile and wave 8 constant-rate (100 MHz) clock stamps, else NULL
};

// Wave priority per phase: s_setprio(3) at the start of stage 1 and after the barrier (slot walk), s_setprio(0) at the node update
// and at the epilogue.  The phases that ISSUE memory requests go ahead of the purely arithmetic node update of other waves -- plain
// f 52.0 -> 50.4 us over four interleaved runs each, fused step unchanged (profiles/r3_ab_prio.txt); the other placements measured
// there were within noise.
// In-kernel phase stamps (diagnostics only; one lane per wave writes s_memtime values)
#ifndef TILE_STAMPS
#define TILE_STAMPS 0   // build with -DTILE_STAMPS=1 for scripts/tile_phases.py (the stamps cost registers and issue slots)
#endif
#if !TILE_STAMPS
#define STAMP(i) do { } while (0)
#else
#define STAMP(i)                                                                                        \
  do {                                                                                                  \
    if (fa.stamps && (threadIdx.x & 63) == 0)                                                           \
      fa.stamps[((int64_t)tile * 4 + (threadIdx.x >> 6)) * 8 + (i)] = (long long)wall_clock64(); \
  } while (0)
#endif
static long long* g_tile_stamps = nullptr;
extern "C" void psignn_prof_tile_stamps(void* d_buf) { g_tile_stamps = (long long*)d_buf; }

// wave sum of the fused epilogue's norm partials: DPP adds inside the rows of 16, row sums through v_readlane (vec_helpers.h)
template <int CTRL>
__device__ __forceinline__ float dpp_perm_f(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
__device__ __forceinline__ float wave_sum_f(float v) {
  v += dpp_perm_f<0xB1>(v);
  v += dpp_perm_f<0x4E>(v);
  v += dpp_perm_f<0x141>(v);
  v += dpp_perm_f<0x140>(v);
  const int vi = __builtin_bit_cast(int, v);   // (the builtin is typed int: a float argument would be converted by value)
  const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(vi, 0));
  const float r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(vi, 16));
  const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(vi, 32));
  const float r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(vi, 48));
  return (r0 + r1) + (r2 + r3);
}

// One tile: body of k_f_tile.  `slot` = position in the launch's tile list.  Every thread of the workgroup reaches the
// stage-1 barrier; returns happen after it (the caller's loop barrier is outside).
template <int P, bool MIXED, bool FUSED, bool MFMA1>
__device__ __forceinline__ void f_tile_body(const FuseArgs& fa, const int slot, const int32_t* __restrict__ tile_list,
                                            const TileCtx* __restrict__ C, const float* __restrict__ W, int lofs, int tofs,
                                            int tnofs, int apply_ln, const float* __restrict__ h,
                                            const int32_t* __restrict__ hsel, int64_t hstride,
                                            const float* __restrict__ h0, const float* __restrict__ prb,
                                            const float* __restrict__ nrm, float* __restrict__ out, float* __restrict__ lds) {
  using L = WLayout<P>;
  constexpr int RS = TileRow<MIXED>::RS;
  const int tile = tile_list ? tile_list[slot] : slot;   // mixed plans: a sub-list of the tiles (see launch_mixed)
  STAMP(0);
  __builtin_amdgcn_s_setprio(3);
  const int tid = threadIdx.x;
  // tile -> node range: arithmetic when the plan's tiles are uniform chunks (always, since round 2; the table stays for
  // tile sizes that are not a multiple of 64)
  const int tn = C->tile_nodes;
  const int32_t t0 = tn ? tile * tn : C->tile_ptr[tile];
  const int n_t = tn ? min(tn, C->n_nodes - t0) : C->tile_ptr[tile + 1] - t0;
  const int n_h = C->halo_cnt[tile];
  const int32_t* hl = C->halo + (int64_t)tile * HALO_CAP;
  if (hsel) h += (int64_t)(*hsel) * hstride;
  if (FUSED) h = fa.xbuf + (int64_t)fa.st[fa.off_cur] * fa.M;

  const float* T = W + tofs;    // transposed section of this layer
  const float* TN = W + tnofs;  // transposed Neumann blocks (mixed)

  // ---- stage 1: neighbour-side projections of tile + halo rows -> LDS
  float x[D];
  if constexpr (MFMA1) {
#if PSIGNN_D == 10
    // Dense node-feature x weight product on the matrix cores: out[row][o] = sum_k x[row][k] W1j[o][k] as
    // v_mfma_f32_16x16x4_f32 tiles with the WEIGHTS as the A operand (A[i = output][k]) and the node rows as B
    // (B[k][j = row]): a lane then receives D[i = 4 (lane>>4) + r][j = lane&15], r = 0..3 -- four consecutive
    // outputs of ONE row -- which is a single 16-byte LDS store.  The f32 MFMA accumulates k in order as an fma
    // chain starting from 0 (MI355X guide, 'FP32-input MFMA'), i.e. the same sum as the VALU form.  K = 10 is
    // padded to 12 (three k-steps), the 20 / 30 outputs to 32 (two M-tiles); 16 rows per N-tile, N-tiles dealt
    // round-robin to the 4 waves.
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    constexpr int NOUT = MIXED ? 30 : 20;
    const int lane = tid & 63, g = lane >> 4, c = lane & 15, wave = tid >> 6;
    float wa[2][3];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int s = 0; s < 3; ++s) {
        const int o = 16 * mt + c, k = 4 * s + g;
        float v = 0.f;
        if (k < D && o < NOUT) {
          const float* blk = o < D ? T + L::T_W1J_TO : (o < 2 * D ? T + L::T_W1J_FR : TN + L::N_W1J);
          v = blk[k * D + (o % D)];
        }
        wa[mt][s] = v;
      }
    const int rows = n_t + n_h;
    for (int nt = wave; nt * 16 < rows; nt += TILE_THREADS / 64) {
      const int row = nt * 16 + c;
      const bool ok = row < rows;
      const int64_t node = !ok ? (int64_t)t0 : (row < n_t ? (int64_t)(t0 + row) : (int64_t)hl[row - n_t]);
      float xb[3];
#pragma unroll
      for (int s = 0; s < 3; ++s) {
        const int k = 4 * s + g;
        float v = 0.f;
        if (ok && k < D) {
          v = h[node * D + k];
          if (FUSED) v += fa.upd[node * D + k];  // x_next = x_cur + update
        }
        xb[s] = v;
      }
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 3; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[mt][s], xb[s], acc, 0, 0, 0);
        const int o0 = 16 * mt + 4 * g;
        if (ok && o0 < (MIXED ? RS : NOUT))
          *reinterpret_cast<float4*>(lds + row * RS + o0) = make_float4(acc[0], acc[1], acc[2], acc[3]);
      }
    }
    if (tid < n_t) {  // this lane's own node state for stage 2 (L1/L2-hot: the rows were just read above)
      loadD(h + (int64_t)(t0 + tid) * D, x);
      if (FUSED) {
        float ur[D];
        loadD(fa.upd + (int64_t)(t0 + tid) * D, ur);
#pragma unroll
        for (int o = 0; o < D; ++o) x[o] += ur[o];
      }
    }
#else
    static_assert(!MFMA1, "the matrix-core stage 1 exists at D = 10 only");
#endif
  } else {
  // mixed family: the Phi_neumann projections are only read by Neumann lanes, i.e. in the few boundary tiles -- every
  // other tile skips a third of its stage-1 work
  bool tile_neu = false;
  if (MIXED) tile_neu = __syncthreads_or(tid < n_t ? (C->flags_p[t0 + tid] & FLAG_NEUMANN) : 0) != 0;
  // Slot rows requested ahead of stage 2 were measured and removed: all of the wave's rows before stage 1, plain f 64.7 - 65.2 vs
  // 57.5 - 58.2 us (profiles/r2_f_tile_ab_runs.txt); row 0 just before the stage-1 barrier, plain f 53.6 vs 53.2 us, fused step
  // 95.0 vs 90.1 us.
  // own row first: every lane's loads are in flight before any projection starts
  const int32_t hidx_w = (tid >> 6 & 1) * 64 + (tid & 63);   // this lane's halo slot inside a 128-row batch
  int32_t hnode = 0;
  if (hidx_w < n_h) hnode = hl[hidx_w];                        // halo index of the first batch, ahead of its use
  float xr[D], xh[D];
  if (tid < n_t) loadD(h + (int64_t)(t0 + tid) * D, xr);
  // the first batch's halo row is requested before the own row is projected (the phase barriers below would otherwise keep
  // its load behind that arithmetic): one more memory round trip off stage 1's critical path
  if (hidx_w < n_h) {
    loadD(h + (int64_t)hnode * D, xh);
    if (FUSED) {
      float uh[D];
      loadD(fa.upd + (int64_t)hnode * D, uh);
#pragma unroll
      for (int o = 0; o < D; ++o) xh[o] += uh[o];
    }
  }
  if (tid < n_t) {
    if (FUSED) {  // x_next = x_cur + update (line_search with on=False: step 1, solver.py:85-94)
      float ur[D];
      loadD(fa.upd + (int64_t)(t0 + tid) * D, ur);
#pragma unroll
      for (int o = 0; o < D; ++o) xr[o] += ur[o];
    }
#pragma unroll
    for (int o = 0; o < D; ++o) x[o] = xr[o];
    v2f ta[NPAIR], tb[NPAIR];
#pragma unroll
    for (int p = 0; p < NPAIR; ++p) ta[p] = tb[p] = splat(0.f);
    PHASE();
    mv2<D>(T + L::T_W1J_TO, xr, ta);
    PHASE();
    mv2<D>(T + L::T_W1J_FR, xr, tb);
    float* rowp = lds + tid * RS;
    lds_store_row2(rowp, ta, tb);
    if (MIXED && tile_neu) {
#pragma unroll
      for (int p = 0; p < NPAIR; ++p) ta[p] = splat(0.f);
      PHASE();
      mv2<D>(TN + L::N_W1J, xr, ta);
      lds_store_row<2 * D>(rowp, ta);
    }
  }
  // Halo rows.  A tile of 256 nodes has ~110 of them: as whole rows (round 1's loop, measured and removed:
  // profiles/r2_f_tile_ab_runs.txt) they were a second round for waves 0 and 1 only, with the other two waves parked at the
  // barrier (stamps: 4.0 vs 2.5 us in stage 1, 1.7 us of barrier wait).  Shared out as HALF rows instead -- waves 0, 1 project the
  // Phi_to half of halo rows [64 (w & 1), +64), waves 2, 3 the Phi_from half -- every wave does one D x D block per 128 halo
  // rows: the same number of wave instructions, half the critical path.
  {
    const int half = __builtin_amdgcn_readfirstlane(tid >> 7);   // wave-uniform: 0 Phi_to columns, 1 Phi_from columns
    for (int hb = 0; hb < n_h; hb += 128) {
      const int idx = hb + hidx_w;
      if (hb > 0 && idx < n_h) hnode = hl[idx];
      if (idx < n_h) {
        float xr[D];
        if (hb == 0) {
#pragma unroll
          for (int o = 0; o < D; ++o) xr[o] = xh[o];
        } else {
          loadD(h + (int64_t)hnode * D, xr);
          if (FUSED) {
            float ur[D];
            loadD(fa.upd + (int64_t)hnode * D, ur);
#pragma unroll
            for (int o = 0; o < D; ++o) xr[o] += ur[o];
          }
        }
        v2f ta[NPAIR];
#pragma unroll
        for (int p = 0; p < NPAIR; ++p) ta[p] = splat(0.f);
        PHASE();
        float* rowp = lds + (n_t + idx) * RS;
        if (half == 0) {
          mv2<D>(T + L::T_W1J_TO, xr, ta);
          lds_store_row<0>(rowp, ta);   // floats 0..D-1 (D = 10: b128, b128, b64)
        } else {
          mv2<D>(T + L::T_W1J_FR, xr, ta);
          lds_store_row<D>(rowp, ta);   // floats D..2D-1 (D = 10: b64, b128, b128)
        }
      }
    }
    if (MIXED && tile_neu) {   // boundary tiles of the mixed family: Phi_neumann columns of the halo rows
      for (int idx = tid; idx < n_h; idx += TILE_THREADS) {
        const int64_t node = hl[idx];
        float xr[D];
        loadD(h + node * D, xr);
        if (FUSED) {
          float ur[D];
          loadD(fa.upd + node * D, ur);
#pragma unroll
          for (int o = 0; o < D; ++o) xr[o] += ur[o];
        }
        v2f ta[NPAIR];
#pragma unroll
        for (int p = 0; p < NPAIR; ++p) ta[p] = splat(0.f);
        PHASE();
        mv2<D>(TN + L::N_W1J, xr, ta);
        lds_store_row<2 * D>(lds + (n_t + idx) * RS, ta);
      }
    }
  }
  }
  // stage 2's first load -- the node's flag byte -- is requested BEFORE the barrier: it sits on the critical path right behind
  // it (flag -> Dirichlet branch -> slot pointer -> first record), an HBM round trip
  const bool active = tid < n_t;
  const int64_t n = (int64_t)t0 + (active ? tid : 0);
  const uint8_t fl = C->flags_p[n];
  STAMP(1);
  __syncthreads();
  STAMP(2);
  __builtin_amdgcn_s_setprio(3);
  if (!FUSED && tid >= n_t) return;

  // ---- stage 2: one tile node per lane
  float y[D];
  const bool dirichlet = fl & FLAG_DIRICHLET;
  if (dirichlet) {  // Dirichlet rows <- h_initial rows (model.py:298)
    loadD(h0 + n * D, y);
    if (!FUSED) {
      storeD(out + n * D, y);
      return;
    }
  }
  if (!dirichlet && active) {
  const int lane = tid & 63;
  // the wave index is wave-uniform: saying so keeps the slice's slot count and the whole slot-loop control in scalar registers
  const int slice = (tn ? tile * (tn >> 6) : C->tile_slice[tile]) + __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint4* slots = C->ell + (int64_t)C->slice_off[slice] * 64 + lane;
  const int nslots = C->slice_deg[slice];

  // target-side projection (bias included) + neighbour sum
  v2f Pi[NPAIR], S_to[NPAIR], S_fr[NPAIR];
  float deg_in, deg_out;
#pragma unroll
  for (int p = 0; p < NPAIR; ++p) S_to[p] = S_fr[p] = splat(0.f);
  // the node state is not needed during the slot walk: park it in memory (the fused step writes x_next to its slot of the
  // iterate buffer anyway) and read it back afterwards -- ten VGPRs less in the loop
  const float* xsrc = h + n * D;
  if (FUSED) {
    float* xn = fa.xbuf + (int64_t)fa.st[fa.off_nxt] * fa.M + n * D;
    storeD(xn, x);
    xsrc = xn;
  }
  // both edge directions in one slot walk, relu folded into the clamp bit of the last edge fma (tile_helpers.h).  One walk per
  // direction was measured and removed: plain f 62.9 vs 61.5 us, fused step 104 vs 99.5 us.
  {
    v2f Pi2[NPAIR];
    ldD(T + L::T_B1_TO, Pi);
    PHASE();
    mv2<D>(T + L::T_W1I_TO, x, Pi);
    ldD(T + L::T_B1_FR, Pi2);
    PHASE();
    mv2<D>(T + L::T_W1I_FR, x, Pi2);
    PHASE();
    edge_pass_both_clamp<RS, FUSED && !MIXED>(slots, nslots, lds, T + L::T_A_TO, T + L::T_A_FR, Pi, Pi2, S_to, S_fr, deg_in, deg_out);
    PHASE();
  }
  STAMP(3);
  __builtin_amdgcn_s_setprio(0);
  loadD(xsrc, x);

  v2f y2[NPAIR];
  if (MIXED && (fl & FLAG_NEUMANN)) {
    // Phi_neumann (Phi_from type: out-edges) + update_neumann: the row is REPLACED (mixed/psignn/model.py:236,241)
    v2f S_n[NPAIR], hid[NPAIR], gN[NPAIR];
    ldD(TN + L::N_B1, Pi);
#pragma unroll
    for (int p = 0; p < NPAIR; ++p) S_n[p] = splat(0.f);
    PHASE();
    mv2<D>(TN + L::N_W1I, x, Pi);
    edge_pass<RS, 2 * D, SLOT_OUT>(slots, nslots, lds, TN + L::N_A, Pi, S_n);
    ldD(TN + L::N_NB1, hid);
    ldD(TN + L::N_gN, gN);
#pragma unroll
    for (int p = 0; p < NPAIR; ++p) hid[p] = __builtin_elementwise_fma(splat(deg_out), gN[p], hid[p]);
    PHASE();
    mv2<D>(TN + L::N_N1H, x, hid);
    PHASE();
    mv2<D>(TN + L::N_GN, reinterpret_cast<const float*>(S_n), hid);
    float pq[P + 2];
#pragma unroll
    for (int k = 0; k < P; ++k) pq[k] = prb[n * P + k];
    pq[P] = nrm[n * 2];
    pq[P + 1] = nrm[n * 2 + 1];
    PHASE();
    mv2<P + 2>(TN + L::N_N1P, pq, hid);
#pragma unroll
    for (int p = 0; p < NPAIR; ++p) hid[p] = __builtin_elementwise_max(hid[p], splat(0.f));
    ldD(TN + L::N_NB2, y2);
    PHASE();
    mv2<D>(TN + L::N_N2, reinterpret_cast<const float*>(hid), y2);
  } else {
    // gate + update MLP on cat = [h | mp_to | mp_from | prb], with mp_* = W2 S + deg b2 folded in
    const float* Wf = W + lofs + L::L_FOLD;  // this layer's fold vectors of the (shared) alpha gate
    const float* Wa = W + L::AL_W;
    const float* sto = reinterpret_cast<const float*>(S_to);
    const float* sfr = reinterpret_cast<const float*>(S_fr);
    float pq[P];
#pragma unroll
    for (int k = 0; k < P; ++k) pq[k] = prb[n * P + k];
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
    v2f hid[NPAIR], g1[NPAIR], g2[NPAIR], upd[NPAIR];
    ldD(T + L::T_HB, hid);
    ldD(T + L::T_gTO, g1);
    ldD(T + L::T_gFR, g2);
#pragma unroll
    for (int p = 0; p < NPAIR; ++p)
      hid[p] = __builtin_elementwise_fma(splat(deg_in), g1[p], __builtin_elementwise_fma(splat(deg_out), g2[p], hid[p]));
    PHASE();
    mv2<D>(T + L::T_U1H, x, hid);
    PHASE();
    mv2<D>(T + L::T_GTO, sto, hid);
    PHASE();
    mv2<D>(T + L::T_GFR, sfr, hid);
    PHASE();
    mv2<P>(T + L::T_U1P, pq, hid);
#pragma unroll
    for (int p = 0; p < NPAIR; ++p) hid[p] = __builtin_elementwise_max(hid[p], splat(0.f));
    ldD(T + L::T_C2, upd);
    PHASE();
    mv2<D>(T + L::T_U2, reinterpret_cast<const float*>(hid), upd);
#pragma unroll
    for (int p = 0; p < NPAIR; ++p) y2[p] = __builtin_elementwise_fma(splat(al), upd[p], (v2f){x[2 * p], x[2 * p + 1]});
  }
#pragma unroll
  for (int p = 0; p < NPAIR; ++p) {
    y[2 * p] = y2[p].x;
    y[2 * p + 1] = y2[p].y;
  }
  if (apply_ln) {  // LayerNorm(10), eps 1e-5, biased variance, affine (model.py:293)
    float mu = 0.f;
#pragma unroll
    for (int o = 0; o < D; ++o) mu += y[o];
    mu *= (1.f / D);
    float var = 0.f;
#pragma unroll
    for (int o = 0; o < D; ++o) {
      float c = y[o] - mu;
      var = fmaf(c, c, var);
    }
    var *= (1.f / D);
    float rs = 1.f / sqrtf(var + 1e-5f);
#pragma unroll
    for (int o = 0; o < D; ++o) y[o] = fmaf((y[o] - mu) * rs, W[L::LN_G + o], W[L::LN_B + o]);
  }
  }  // !dirichlet && active
  STAMP(4);
  __builtin_amdgcn_s_setprio(0);
  if (!FUSED) {
    storeD(out + n * D, y);
    STAMP(5);
    return;
  }
  // ---- fused Broyden epilogue
  float sg = 0.f, sf = 0.f;
  if (active) {
    float gn[D];
#pragma unroll
    for (int o = 0; o < D; ++o) {
      gn[o] = y[o] - x[o];
      sg = fmaf(gn[o], gn[o], sg);
      sf = fmaf(y[o], y[o], sf);
    }
    storeD(fa.gnew + n * D, gn);
    if (dirichlet) storeD(fa.xbuf + (int64_t)fa.st[fa.off_nxt] * fa.M + n * D, x);
  }
  // one partial pair per tile: wave shuffles, then the 4 wave sums through LDS in a fixed order
  sg = wave_sum_f(sg);
  sf = wave_sum_f(sf);
  __shared__ float red[2][4];
  if ((tid & 63) == 0) {
    red[0][tid >> 6] = sg;
    red[1][tid >> 6] = sf;
  }
  __syncthreads();
  if (tid == 0) {
    fa.part[tile] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    fa.part[fa.npart + tile] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
  }
}

// Kernel: one workgroup per tile.  blocks b and b+8 share an XCD (round-robin dispatch): each XCD owns a contiguous run of
// `chunk` tiles, so that neighbouring tiles' halo rows hit the same L2.  Speed only; any mapping is correct.
// (Round 2 tried persistent workgroups -- a grid of 5 per CU striding through the XCD's run, and the same with a per-XCD
// atomic work queue whose next index is fetched during the current tile -- to fill the tail the phase stamps show: 60.9 - 62.2
// and 62.6 - 64.8 us against 57.7 - 58.7 us for this form on the 1M-node mesh; the loop state also cost the fused variant its
// fifth wave.  Removed; profiles/r2_f_tile_ab_runs.txt keeps the runs.)
// The tile pointers travel as a by-value struct in the kernel arguments.  Passing them behind a device pointer was measured and
// removed (profiles/r2_f_tile_ab_runs.txt): plain f 54.9 - 57.7 vs 52.6 - 53.9 us, fused step 97.7 vs 94.0 us.
template <int P, bool MIXED, bool FUSED, bool MFMA1>
__global__ __launch_bounds__(TILE_THREADS) void k_f_tile(FuseArgs fa, int n_tiles, int chunk, const int32_t* __restrict__ tile_list,
                                                const TileCtx Cv, const float* __restrict__ W, int lofs, int tofs,
                                                int tnofs, int apply_ln, const float* __restrict__ h,
                                                const int32_t* __restrict__ hsel, int64_t hstride,
                                                const float* __restrict__ h0, const float* __restrict__ prb,
                                                const float* __restrict__ nrm, float* __restrict__ out) {
  const TileCtx* __restrict__ C = &Cv;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  if (FUSED && fa.st[fa.off_done]) return;
  const int slot = xcd_tile_slot(chunk);
  if (slot >= n_tiles) return;
  f_tile_body<P, MIXED, FUSED, MFMA1>(fa, slot, tile_list, C, W, lofs, tofs, tnofs, apply_ln, h, hsel, hstride, h0, prb, nrm, out,
                                      lds);
}

static unsigned tile_grid(int chunk);

// Batched fused Broyden step (solver.hip psignn_broyden_solve_batch; dirichlet, single layer): ONE launch evaluates the
// fused step of every mesh of a shard.  The tiles of all meshes form one list (mesh m owns slots [tile_base[m],
// tile_base[m] + n_tiles[m])); a workgroup looks its slot's mesh up, loads that mesh's pointers from its descriptor and runs
// the same tile body as the single-mesh kernel -- same arithmetic per node, same per-tile norm partials.  A mesh whose stop
// test has fired is skipped tile by tile.
template <int P, bool MIXED>
__global__ __launch_bounds__(TILE_THREADS) void k_f_tile_batch(const BatchDesc* __restrict__ descs, int n_mesh, int n_slots, int chunk,
                                                              int off_done, int off_cur, int off_nxt, int par,
                                                              const float* __restrict__ W, int lofs, int tofs, int tnofs) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int slot = xcd_tile_slot(chunk);
  if (slot >= n_slots) return;
  int m = 0;
  while (m + 1 < n_mesh && descs[m + 1].tile_base <= slot) ++m;   // wave-uniform scalar walk (a shard has few meshes)
  const BatchDesc& d = descs[m];
  if (d.st[off_done]) return;
  FuseArgs fa{d.upd, par ? d.g0 : d.g1, d.xbuf, d.st, off_done, off_cur, off_nxt, d.M, d.nrm_part, d.n_tiles, nullptr};
  f_tile_body<P, MIXED, true, false>(fa, slot - d.tile_base, nullptr, d.ctx, W, lofs, tofs, tnofs, 1, d.xbuf, nullptr, 0, d.h0p, d.prbp,
                                     d.nrmp, nullptr, lds);
}

// descs: device array of n_mesh descriptors; max_rows: largest tile + halo row count over the meshes (LDS size).
// mixed shards: every tile runs the full kernel (128-byte LDS rows, Neumann branch for the lanes that need it) in tile order --
// what the single-mesh fused step does below 2 048 plain tiles, and bit-identical to its two-group launch above that
// (tests/test_gpu_configs.py::test_mixed_two_group_launch_at_natural_size).
int psignn_f_tile_fused_batch(const BatchDesc* d_descs, int n_mesh, int n_slots, int max_rows, const float* W, int mixed,
                              int off_done, int off_cur, int off_nxt, int par, hipStream_t st) {
  const int chunk = (int)cdiv(n_slots, 8);
  if (mixed) {
    using L = WLayout<3>;
    LAUNCH("k_f_tile_fused", st, (k_f_tile_batch<3, true><<<tile_grid(chunk), TILE_THREADS, (size_t)max_rows * TileRow<true>::RS * 4, st>>>(
        d_descs, n_mesh, n_slots, chunk, off_done, off_cur, off_nxt, par, W, L::layer(0), L::tp_layer(1, true, 0), L::tp_neu(1))));
  } else {
    using L = WLayout<2>;
    LAUNCH("k_f_tile_fused", st, (k_f_tile_batch<2, false><<<tile_grid(chunk), TILE_THREADS, (size_t)max_rows * TileRow<false>::RS * 4, st>>>(
        d_descs, n_mesh, n_slots, chunk, off_done, off_cur, off_nxt, par, W, L::layer(0), L::tp_layer(1, false, 0), 0)));
  }
  HIP_TRY(hipGetLastError());
  return PSIGNN_OK;
}

// Batched plain f (fpiter.hip psignn_anderson_solve_batch / psignn_picard_solve_batch; single layer, LayerNorm applied): ONE launch
// evaluates f of every mesh of a shard at ring row `in_row` of its X (in_f = 0) or F (in_f = 1) slots and writes the mesh's fx row.
// The slot list and the descriptor walk are k_f_tile_batch's; the tile body is the plain single-mesh kernel's, so every mesh has the
// bits of psignn_f_forward_p on its own plan.  A mesh whose stop test has fired is skipped tile by tile.
template <int P, bool MIXED>
__global__ __launch_bounds__(TILE_THREADS) void k_f_tile_plain_batch(const FpBatchDesc* __restrict__ descs, int n_mesh, int n_slots,
                                                                    int chunk, int off_done, int in_f, int in_row,
                                                                    const float* __restrict__ W, int lofs, int tofs, int tnofs) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int slot = xcd_tile_slot(chunk);
  if (slot >= n_slots) return;
  int m = 0;
  while (m + 1 < n_mesh && descs[m + 1].tile_base <= slot) ++m;   // wave-uniform scalar walk (a shard has few meshes)
  const FpBatchDesc& d = descs[m];
  if (d.st32[off_done]) return;
  const float* h = (in_f ? d.F : d.X) + (int64_t)in_row * d.ld;
  f_tile_body<P, MIXED, false, false>(FuseArgs{}, slot - d.tile_base, nullptr, d.ctx, W, lofs, tofs, tnofs, 1, h, nullptr, 0, d.h0p,
                                      d.prbp, d.nrmp, d.fx, lds);
}

// Dynamic LDS beyond 64 KiB is asked for once per device (width 16: 768 rows of a dirichlet tile are 98 304 B); the largest request a
// tiled plan can make, so that one grant serves every shard.
static bool plain_batch_lds_granted() {
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return false;
  static int state[64] = {0};   // 0 unknown, 1 granted, -1 refused
  if (state[dev] == 0) {
    const int want_d = (TILE_MAX + HALO_CAP) * TileRow<false>::RS * 4, want_m = MIXED_ROW_CAP * TileRow<true>::RS * 4;
    const bool ok =
        hipFuncSetAttribute((const void*)k_f_tile_plain_batch<2, false>, hipFuncAttributeMaxDynamicSharedMemorySize, want_d) == hipSuccess &&
        hipFuncSetAttribute((const void*)k_f_tile_plain_batch<3, true>, hipFuncAttributeMaxDynamicSharedMemorySize, want_m) == hipSuccess;
    if (!ok) (void)hipGetLastError();
    state[dev] = ok ? 1 : -1;
  }
  return state[dev] > 0;
}

// descs: device array of n_mesh descriptors; max_rows: largest tile + halo row count over the meshes (LDS size).  Mixed shards run the
// full kernel in tile order, as psignn_f_tile_fused_batch does.  Records as the single-mesh plain launch does ("k_f_tile").
int psignn_f_tile_plain_batch(const FpBatchDesc* d_descs, int n_mesh, int n_slots, int max_rows, const float* W, int mixed, int off_done,
                              int in_f, int in_row, hipStream_t st) {
  const int chunk = (int)cdiv(n_slots, 8);
  const size_t lds = (size_t)max_rows * (mixed ? TileRow<true>::RS : TileRow<false>::RS) * 4;
  ARG_CHECK(max_rows > 0 && max_rows <= (mixed ? MIXED_ROW_CAP : TILE_MAX + HALO_CAP), "tile rows beyond the plan's limits");
  if (lds > 64 * 1024 && !plain_batch_lds_granted()) {
    psignn_set_error("batched plain f: %zu bytes of dynamic LDS were refused", lds);
    return PSIGNN_EHIP;
  }
  if (mixed) {
    using L = WLayout<3>;
    LAUNCH("k_f_tile", st, (k_f_tile_plain_batch<3, true><<<tile_grid(chunk), TILE_THREADS, lds, st>>>(
        d_descs, n_mesh, n_slots, chunk, off_done, in_f, in_row, W, L::layer(0), L::tp_layer(1, true, 0), L::tp_neu(1))));
  } else {
    using L = WLayout<2>;
    LAUNCH("k_f_tile", st, (k_f_tile_plain_batch<2, false><<<tile_grid(chunk), TILE_THREADS, lds, st>>>(
        d_descs, n_mesh, n_slots, chunk, off_done, in_f, in_row, W, L::layer(0), L::tp_layer(1, false, 0), 0)));
  }
  HIP_TRY(hipGetLastError());
  return PSIGNN_OK;
}

// gather of node rows between the caller's numbering and the plan order: dst[i] = src[map[i]]
__global__ void k_permute_rows(int64_t N, int cols, const int32_t* __restrict__ map, const float* __restrict__ src,
                               float* __restrict__ dst) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N * cols) return;
  int64_t r = i / cols, c = i - r * cols;
  dst[i] = src[(int64_t)map[r] * cols + c];
}

// ------------------------------------------------------------------------------------------ host
// Grid of a tile-kernel launch over `chunk` tiles per XCD: one workgroup per tile, a multiple of 8.
static unsigned tile_grid(int chunk) { return (unsigned)(chunk * 8); }

static FuseArgs plain_args() {
  FuseArgs a{};
  a.stamps = g_tile_stamps;
  return a;
}

// Mixed family: two launches over disjoint tile groups.  Tiles without Neumann nodes (all but the boundary tiles) run the
// kernel WITHOUT the Neumann branch and with 80-byte LDS rows (the Phi_neumann columns are only read by Neumann lanes);
// the few tiles with Neumann nodes run the full kernel with 128-byte rows.  Same arithmetic per node either way.
template <bool FUSED>
static void launch_mixed(const psignn_plan* p, const FuseArgs& fa, const char* name, const float* W, int nl, const float* h,
                         const int32_t* hsel, int64_t hstride, const float* h0, const float* prb, const float* nrm,
                         float* out, hipStream_t st) {
  using L = WLayout<3>;
  const int lofs = L::layer(nl - 1), tofs = L::tp_layer(nl, true, nl - 1), tnofs = L::tp_neu(nl);
  int na = (int)p->n_tiles_plain, nb = (int)(p->n_tiles - p->n_tiles_plain);
  // the second launch costs ~10 us of latency: worth it only when the first group is long (1M nodes: plain f 99 -> 82 us;
  // 100 k nodes: 3 % slower per Broyden iteration) -- below 2 048 plain tiles everything runs in the full kernel
  const char* e = getenv("PSIGNN_MIXED_SPLIT_MIN");   // tests force the two-group path on small meshes with 0
  if (na < (e ? atoi(e) : 2048)) {
    na = 0;
    nb = (int)p->n_tiles;
  }
  const int32_t* list_b = na > 0 ? p->tile_order + na : nullptr;
  if (na > 0) {
    const int chunk = (int)cdiv(na, 8);
    LAUNCH(name, st, (k_f_tile<3, false, FUSED, false><<<tile_grid(chunk), TILE_THREADS, (size_t)p->max_rows * TileRow<false>::RS * 4, st>>>(
        fa, na, chunk, p->tile_order, p->h_ctx, W, lofs, tofs, tnofs, 1, h, hsel, hstride, h0, prb, nrm, out)));
  }
  if (nb > 0) {
    const int chunk = (int)cdiv(nb, 8);
    LAUNCH(name, st, (k_f_tile<3, true, FUSED, false><<<tile_grid(chunk), TILE_THREADS, (size_t)p->max_rows * TileRow<true>::RS * 4, st>>>(
        fa, nb, chunk, list_b, p->h_ctx, W, lofs, tofs, tnofs, 1, h, hsel, hstride, h0, prb, nrm, out)));
  }
}

// All tensors in plan order.  h = hbase + (*hsel) * hstride when hsel != NULL.
int psignn_f_tile_forward(const psignn_plan* p, const float* W, int nl, const float* h, const int32_t* hsel,
                          int64_t hstride, const float* h0, const float* prb, const float* nrm, float* out,
                          float* work, hipStream_t st) {
  ARG_CHECK(p && p->tiled, "plan has no tile structures");
  ARG_CHECK(W && h && h0 && prb && out, "NULL argument");
  ARG_CHECK(!p->mixed || nrm, "mixed plan needs unit normals");
  const int chunk = (int)cdiv(p->n_tiles, 8);
  const unsigned grid = tile_grid(chunk);
  // B_f: h, h' (40 N each), prb (8 / 12 N), flags and, mixed, normals; 20 bytes per directed non-self edge
  PROF_BYTES(((p->mixed ? 8 * D + 22 : 8 * D + 9) * p->N + 20 * p->Ep) * (p->mixed ? 1 : nl));   // 102 / 89 N at D = 10
  if (p->mixed) {
    using L = WLayout<3>;
    if (stage1_mfma(false, true)) {  // single launch, MFMA stage 1 (PSIGNN_STAGE1=mfma)
      size_t lds = (size_t)p->max_rows * TileRow<true>::RS * 4;
      LAUNCH("k_f_tile", st, (k_f_tile<3, true, false, MFMA_FORM><<<grid, TILE_THREADS, lds, st>>>(
        plain_args(), (int)p->n_tiles, chunk, nullptr, p->h_ctx, W, L::layer(nl - 1), L::tp_layer(nl, true, nl - 1), L::tp_neu(nl), 1,
        h, hsel, hstride, h0, prb, nrm, out)));
    } else {
      launch_mixed<false>(p, plain_args(), "k_f_tile", W, nl, h, hsel, hstride, h0, prb, nrm, out, st);
    }
  } else {
    using L = WLayout<2>;
    size_t lds = (size_t)p->max_rows * TileRow<false>::RS * 4;
    ARG_CHECK(nl == 1 || work, "multi-layer evaluation needs a workspace");
    const ws::FFwd ft = ws::f_fwd(p->N, true, work, 0);   // NULL without a workspace (single layer)
    float* const* pp = ft.pp;
    const float* cur = h;
    for (int l = 0; l < nl; ++l) {
      float* dst = (l == nl - 1) ? out : pp[l & 1];
      if (stage1_mfma(false, false))
        LAUNCH("k_f_tile", st, (k_f_tile<2, false, false, MFMA_FORM><<<grid, TILE_THREADS, lds, st>>>(
            plain_args(), (int)p->n_tiles, chunk, nullptr, p->h_ctx, W, L::layer(l), L::tp_layer(nl, false, l), 0, l == nl - 1, cur,
            l == 0 ? hsel : nullptr, hstride, h0, prb, nrm, dst)));
      else
        LAUNCH("k_f_tile", st, (k_f_tile<2, false, false, false><<<grid, TILE_THREADS, lds, st>>>(
            plain_args(), (int)p->n_tiles, chunk, nullptr, p->h_ctx, W, L::layer(l), L::tp_layer(nl, false, l), 0, l == nl - 1, cur,
            l == 0 ? hsel : nullptr, hstride, h0, prb, nrm, dst)));
      cur = dst;
    }
  }
  HIP_TRY(hipGetLastError());
  return PSIGNN_OK;
}

// Layer l of a dirichlet block at its own input state h (plan order; h0: the Dirichlet rows written after the layer):
// the layer states a multi-layer derivative differentiates at (fgnn_layers.hip).  LayerNorm on the last layer only;
// the same launches as the layer loop of psignn_f_tile_forward, so the states are bit-identical to the forward's.
int psignn_f_tile_layer(const psignn_plan* p, const float* W, int nl, int l, const float* h, const float* h0, const float* prb,
                        float* out, hipStream_t st) {
  ARG_CHECK(p && p->tiled && !p->mixed && l >= 0 && l < nl, "tiled layer: dirichlet plans, 0 <= layer < n_layers");
  ARG_CHECK(W && h && h0 && prb && out && out != h, "bad arguments");
  using L = WLayout<2>;
  const int chunk = (int)cdiv(p->n_tiles, 8);
  const unsigned grid = tile_grid(chunk);
  size_t lds = (size_t)p->max_rows * TileRow<false>::RS * 4;
  PROF_BYTES((8 * D + 9) * p->N + 20 * p->Ep);   // B_f of one layer (psignn_f_tile_forward)
  if (stage1_mfma(false, false))
    LAUNCH("k_f_tile_layer", st, (k_f_tile<2, false, false, MFMA_FORM><<<grid, TILE_THREADS, lds, st>>>(
        plain_args(), (int)p->n_tiles, chunk, nullptr, p->h_ctx, W, L::layer(l), L::tp_layer(nl, false, l), 0, l == nl - 1, h,
        nullptr, 0, h0, prb, nullptr, out)));
  else
    LAUNCH("k_f_tile_layer", st, (k_f_tile<2, false, false, false><<<grid, TILE_THREADS, lds, st>>>(
        plain_args(), (int)p->n_tiles, chunk, nullptr, p->h_ctx, W, L::layer(l), L::tp_layer(nl, false, l), 0, l == nl - 1, h,
        nullptr, 0, h0, prb, nullptr, out)));
  HIP_TRY(hipGetLastError());
  return PSIGNN_OK;
}

// Fused Broyden step (single-layer models): x_next = x_cur + upd, f(x_next), g_new / x_next / norm partials.
// Returns the number of partial entries per norm (n_tiles), or a negative error.
int psignn_f_tile_fused(const psignn_plan* p, const float* W, int nl, float* xbuf, int64_t M, const int32_t* st_words,
                        int off_done, int off_cur, int off_nxt, const float* upd, float* gnew,
                        const float* h0, const float* prb, const float* nrm, float* part, hipStream_t st) {
  ARG_CHECK(p && p->tiled, "plan has no tile structures");
  ARG_CHECK(nl == 1 || p->mixed, "fused step supports single-layer evaluation");
  const int chunk = (int)cdiv(p->n_tiles, 8);
  const unsigned grid = tile_grid(chunk);
  const int npart = (int)p->n_tiles;
  FuseArgs fa{upd, gnew, xbuf, st_words, off_done, off_cur, off_nxt, M, part, npart, g_tile_stamps};
  PROF_BYTES((p->mixed ? 8 * D + 22 : 8 * D + 9) * p->N + 20 * p->Ep + 8 * M);   // B_f + update read, g_new written (x_next replaces f(x))
  if (p->mixed) {
    using L = WLayout<3>;
    if (stage1_mfma(true, true)) {
      size_t lds = (size_t)p->max_rows * TileRow<true>::RS * 4;
      LAUNCH("k_f_tile_fused", st, (k_f_tile<3, true, true, MFMA_FORM><<<grid, TILE_THREADS, lds, st>>>(
        fa, (int)p->n_tiles, chunk, nullptr, p->h_ctx, W, L::layer(nl - 1), L::tp_layer(nl, true, nl - 1), L::tp_neu(nl), 1, xbuf,
        nullptr, 0, h0, prb, nrm, nullptr)));
    } else {
      launch_mixed<true>(p, fa, "k_f_tile_fused", W, nl, xbuf, nullptr, 0, h0, prb, nrm, nullptr, st);
    }
  } else {
    using L = WLayout<2>;
    size_t lds = (size_t)p->max_rows * TileRow<false>::RS * 4;
    if (stage1_mfma(true, false))
      LAUNCH("k_f_tile_fused", st, (k_f_tile<2, false, true, MFMA_FORM><<<grid, TILE_THREADS, lds, st>>>(
        fa, (int)p->n_tiles, chunk, nullptr, p->h_ctx, W, L::layer(0), L::tp_layer(nl, false, 0), 0, 1, xbuf, nullptr, 0, h0, prb, nrm,
        nullptr)));
    else
      LAUNCH("k_f_tile_fused", st, (k_f_tile<2, false, true, false><<<grid, TILE_THREADS, lds, st>>>(
        fa, (int)p->n_tiles, chunk, nullptr, p->h_ctx, W, L::layer(0), L::tp_layer(nl, false, 0), 0, 1, xbuf, nullptr, 0, h0, prb, nrm,
        nullptr)));
  }
  HIP_TRY(hipGetLastError());
  return npart;
}

// dst[new] = src[perm[new]]  (to_plan = 1)   or   dst[old] = src[inv[old]]  (to_plan = 0); rows of `cols` floats
extern "C" int psignn_plan_permute(const psignn_plan_t* p, const float* src, int cols, float* dst, int to_plan, void* stream) {
  ARG_CHECK(p && src && dst && cols > 0, "bad arguments");
  ARG_CHECK(src != dst, "in-place permutation is not supported");
  hipStream_t st = (hipStream_t)stream;
  if (!p->tiled) {
    HIP_TRY(hipMemcpyAsync(dst, src, (size_t)p->N * cols * 4, hipMemcpyDeviceToDevice, st));
    return PSIGNN_OK;
  }
  int64_t n = p->N * cols;
  k_permute_rows<<<(unsigned)cdiv(n, 256), 256, 0, st>>>(p->N, cols, to_plan ? p->perm : p->inv, src, dst);
  HIP_TRY(hipGetLastError());
  return PSIGNN_OK;
}
