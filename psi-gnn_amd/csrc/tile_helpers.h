// The one device header of every tile kernel (fgnn_tile, fgnn_tile_jvp, fgnn_tile_vjp, fgnn_tile_jr, fgnn_tile_lin, dsgps_tile,
// dss_tile; gfx950): packed-fp32 matvecs on the transposed weight blocks, the XCD tile-slot order, and the pieces of a walk over
// the pair-merged slots of one edge direction -- the pipelined walk itself (SlotWalk), the LDS row loader (lds_row / lds_row8)
// and the edge pre-activation (ld_attr, slot_attr, edge_preact).
#pragma once
#include "fgnn_common.h"

#define SLOT_IN 0x10000u
#define SLOT_OUT 0x20000u

// Packed fp32: CDNA issues one VALU instruction per wave every 4 cycles; v_pk_fma_f32 / v_pk_add_f32 carry two
// floats per lane in that slot, so the FP32 peak (and this kernel, which is VALU-issue bound) needs them.  All
// matrices are read from the transposed weight section ([in k][out o], o fastest): the outputs (2p, 2p+1) of one
// input k sit in one SGPR pair.  Each output is still the same k-ordered fma chain as in fgnn.hip.
// Workgroup = 4 waves = TILE_MAX lanes.  (A fifth wave that only helps with the halo rows of stage 1 was tried:
// 79 us instead of 67 us per 1M-node evaluation -- it costs a wave slot per workgroup for the whole residency.)
#define TILE_THREADS 256
#define EDGE_PD 2   // prefetch distance of the slot loads of every single-direction walk (SlotWalk)

typedef float v2f __attribute__((ext_vector_type(2)));

__device__ __forceinline__ v2f splat(float a) { return (v2f){a, a}; }

// acc[p] += WT[k][2p..2p+1] * x[k],  p < NPAIR (= D / 2: 5 at the default width), k < K
// A 10 x 10 block is 100 wave-uniform weights (D x D in general) -- with the wave's other live SGPRs more than the 102 there are, and the
// compiler, which loads a whole block ahead of its first use, then parks the excess in VGPR lanes (v_writelane /
// v_readlane: 36 VALU slots per stage-1 round in round 1's build).  A compiler barrier every MV2_CH inputs keeps at most
// MV2_CH x 10 weights in flight.  MV2_CH 0 (fgnn_tile_vjp.hip): no chunk barriers, the caller's PHASE() per product is the bound.
#ifndef MV2_CH
#define MV2_CH 5
#endif
// MV2_LAUNDER (round 3): the barrier alone does not hold the loads back -- the weights sit behind a `const __restrict__` kernel
// argument, their loads are invariant for the optimiser and were still hoisted over it: the fused f step and k_jvp_lin carried
// 220 / 204 v_writelane / v_readlane per wave (a sixth of their VALU instructions) for parked weights.  Adding an
// offset that went through an empty asm (always 0) to the block's pointer per chunk makes the chunk's loads data-dependent on
// that statement: they cannot move above it.  (Laundering the pointer itself loses its no-alias property: vector loads, 256 VGPRs.)
#ifndef MV2_LAUNDER
#define MV2_LAUNDER 0   // 0: barrier only; 2: offset re-made per chunk by a statement that also waits for the chunk before.  Chosen per
                        // file (fgnn_tile.hip, fgnn_tile_lin.hip: 2); which form leaves fewest parked SGPRs differs from kernel to kernel.
                        // The offset re-made without the wait was measured and removed (profiles/r3_ab_mv2.txt, MV2_LAUNDER=1).
#endif
template <int K>
__device__ __forceinline__ void mv2(const float* __restrict__ WT, const float* x, v2f* acc, const float after = 0.f) {
  const v2f* w = reinterpret_cast<const v2f*>(WT);
#if MV2_LAUNDER
  // An offset the optimiser cannot see through (always 0; the POINTER stays derived from the restrict argument: scalar loads),
  // re-made per chunk by a statement that also consumes the accumulators of the chunk before -- the chunk's loads can neither be
  // hoisted over it nor can the statement itself float above the arithmetic it waits for.  `after`: a value of the caller's that
  // the first chunk has to wait for (e.g. the last output of an independent product issued just before).
  int zero = 0;
  asm volatile("" : "+s"(zero) : "v"(acc[0]), "v"(acc[NPAIR - 1]), "v"(after));
  w += zero;
#endif
#pragma unroll
  for (int k = 0; k < K; ++k) {
    if (MV2_CH > 0 && k > 0 && k % (MV2_CH > 0 ? MV2_CH : 1) == 0) {   // (MV2_CH 0: no chunk barriers)
      PHASE();
#if MV2_LAUNDER
      asm volatile("" : "+s"(zero) : "v"(acc[0]), "v"(acc[NPAIR - 1]));
      w += zero;
#endif
    }
    const v2f xs = splat(x[k]);
#pragma unroll
    for (int p = 0; p < NPAIR; ++p) acc[p] = __builtin_elementwise_fma(w[k * NPAIR + p], xs, acc[p]);
  }
}
__device__ __forceinline__ void ldD(const float* __restrict__ p, v2f* r) {  // D wave-uniform floats (8-byte aligned): NPAIR pairs
  const v2f* q = reinterpret_cast<const v2f*>(p);
#pragma unroll
  for (int i = 0; i < NPAIR; ++i) r[i] = q[i];
}
__device__ __forceinline__ void ld5(const float* __restrict__ p, v2f* r) { ldD(p, r); }   // its name in the width-10-only files
// pair i of a row held as 16-byte quads: (x, y) of quad i / 2 for even i, (z, w) for odd i
__device__ __forceinline__ v2f quad_pair(const float4* v, int i) {
  return (i & 1) ? (v2f){v[i >> 1].z, v[i >> 1].w} : (v2f){v[i >> 1].x, v[i >> 1].y};
}

// Workgroup b of a grid of 8 * chunk runs tile slot (b & 7) * chunk + (b >> 3): workgroups are dealt round-robin to the eight
// XCDs, so each XCD's L2 sees one contiguous run of `chunk` tiles.
__host__ __device__ __forceinline__ unsigned xcd_slot(unsigned b, int chunk) { return (b & 7) * chunk + (b >> 3); }
__device__ __forceinline__ unsigned xcd_tile_slot(int chunk) { return xcd_slot(blockIdx.x, chunk); }

// ---- the pieces of a single-direction slot walk ------------------------------------------------------------------
// D floats of an LDS row as NPAIR pairs: row (16-byte aligned) + COL.  The column is a template parameter so that the
// choice between the two load shapes is made at compile time.
template <int COL>
__device__ __forceinline__ void lds_row(const float* __restrict__ row, v2f* pj) {
  row += COL;
  if (COL % 4 == 0) {  // 16-byte aligned start: D / 4 b128 and, when D is not a multiple of 4, a b64 (D = 10: b128, b128, b64)
    float4 v[D / 4];
#pragma unroll
    for (int q = 0; q < D / 4; ++q) v[q] = reinterpret_cast<const float4*>(row)[q];
#pragma unroll
    for (int p = 0; p < D / 4 * 2; ++p) pj[p] = quad_pair(v, p);
    if (D % 4) {
      float2 t = reinterpret_cast<const float2*>(row)[NPAIR - 1];
      pj[NPAIR - 1] = (v2f){t.x, t.y};
    }
  } else {             // start at 8 mod 16 (D = 2 mod 4 only): b64, then D / 4 b128 (D = 10: b64, b128, b128)
    static_assert(COL % 4 == 0 || D % 4 == 2, "a row segment starting at 8 mod 16 has 4 q + 2 floats");
    float2 t = reinterpret_cast<const float2*>(row)[0];
    float4 v[D / 4];
#pragma unroll
    for (int q = 0; q < D / 4; ++q) v[q] = reinterpret_cast<const float4*>(row + 2)[q];
    pj[0] = (v2f){t.x, t.y};
#pragma unroll
    for (int p = 0; p < D / 4 * 2; ++p) pj[1 + p] = quad_pair(v, p);
  }
}
// the same from a row that is only 8-byte aligned (120-byte rows): NPAIR b64
__device__ __forceinline__ void lds_row8(const float* __restrict__ row, v2f* pj) {
#pragma unroll
  for (int i = 0; i < NPAIR; ++i) {
    const float2 t = reinterpret_cast<const float2*>(row)[i];
    pj[i] = (v2f){t.x, t.y};
  }
}

// the attr block AT (3 x D wave-uniform floats, transposed) of one Phi module
__device__ __forceinline__ void ld_attr(const float* __restrict__ AT, v2f* wa) {
#pragma unroll
  for (int i = 0; i < 3 * NPAIR; ++i) wa[i] = reinterpret_cast<const v2f*>(AT)[i];
}
// the attr (a0, a1, a2) of a slot, each splat over a pair; the reverse passes multiply `flip` into a0, a1 before the splat
struct SlotAttr { v2f a0, a1, a2; };
__device__ __forceinline__ SlotAttr slot_attr(const uint4& s) {
  return {splat(__uint_as_float(s.y)), splat(__uint_as_float(s.z)), splat(__uint_as_float(s.w))};
}
__device__ __forceinline__ SlotAttr slot_attr(const uint4& s, float flip) {
  return {splat(flip * __uint_as_float(s.y)), splat(flip * __uint_as_float(s.z)), splat(__uint_as_float(s.w))};
}
// z = x + y + AT . (a0, a1, a2): NPAIR independent chains, written stage by stage so that dependent packed ops are never back
// to back
__device__ __forceinline__ void edge_preact(const v2f* wa, const SlotAttr& a, const v2f* x, const v2f* y, v2f* z) {
#pragma unroll
  for (int p = 0; p < NPAIR; ++p) z[p] = x[p] + y[p];
#pragma unroll
  for (int p = 0; p < NPAIR; ++p) z[p] = __builtin_elementwise_fma(wa[p], a.a0, z[p]);
#pragma unroll
  for (int p = 0; p < NPAIR; ++p) z[p] = __builtin_elementwise_fma(wa[NPAIR + p], a.a1, z[p]);
#pragma unroll
  for (int p = 0; p < NPAIR; ++p) z[p] = __builtin_elementwise_fma(wa[2 * NPAIR + p], a.a2, z[p]);
}

// The walk over this lane's slots, as the state of a for loop:
//   for (SlotWalk<PD, MASK> w(slots, nslots); w.more(); w.step())
//     if (w.live()) { ... w.slot() ... w.row() ... }
// live(): the current slot is not empty and carries MASK; row(): its LDS row index.  Software pipeline of distance PD (at
// PD = 2: c0, c1, then nx = slots[min(r + 2, nslots - 1) * 64]): the 16-byte slot loads are unconditional (index clamped,
// never branched on) so the compiler keeps them whole and places their waits PD - 1 iterations later.  (A struct of scalars and
// not a callable: a closure holds the addresses of the caller's accumulator arrays, which kept them in scratch memory in the
// walk with two weight blocks, pass_rev_in_mixed.)
template <int PD, unsigned MASK>
struct SlotWalk {
  const uint4* __restrict__ slots;
  int nslots, r;
  uint4 c[PD], nx;
  __device__ __forceinline__ SlotWalk(const uint4* __restrict__ slots_, int nslots_) : slots(slots_), nslots(nslots_), r(0) {
    if (nslots <= 0) return;
#pragma unroll
    for (int i = 0; i < PD; ++i) c[i] = slots[(int64_t)min(i, nslots - 1) * 64];
  }
  __device__ __forceinline__ bool more() {   // also issues the load PD slots ahead
    if (r >= nslots) return false;
    nx = slots[(int64_t)min(r + PD, nslots - 1) * 64];
    return true;
  }
  __device__ __forceinline__ bool live() const { return (c[0].x & 0xFFFFu) != ELL_EMPTY && (c[0].x & MASK); }
  __device__ __forceinline__ const uint4& slot() const { return c[0]; }
  __device__ __forceinline__ int row() const { return (int)(c[0].x & 0xFFFFu); }
  __device__ __forceinline__ void step() {
#pragma unroll
    for (int i = 0; i + 1 < PD; ++i) c[i] = c[i + 1];
    c[PD - 1] = nx;
    ++r;
  }
};

// One direction of the neighbour sum for this lane's node:
//   S[o] += relu(Pi[o] + row[COL + o] + AT[:, o] . (a0, a1, a2))   over the slots that carry `MASK`
// (AT = W1[:, 20:23]^T; for in-edges its first two rows are stored negated, because an in-edge's attr is the
// mirror (-a0, -a1, a2) of the slot's attr).  The two directions are separate passes on purpose: one pass needs
// 30 wave-uniform weights, which stay in SGPRs across the loop; with 60 the compiler re-issues the scalar loads
// and their waits in every iteration.  The second pass re-reads the 16-byte slots from L1/L2.
template <int RS, int COL, unsigned MASK>
__device__ __forceinline__ float edge_pass(const uint4* __restrict__ slots, int nslots, const float* __restrict__ lds,
                                           const float* __restrict__ AT, const v2f* Pi, v2f* S) {
  float deg = 0.f;
  v2f wa[3 * NPAIR];
  ld_attr(AT, wa);
  for (SlotWalk<EDGE_PD, MASK> w(slots, nslots); w.more(); w.step())
    if (w.live()) {
      const SlotAttr a = slot_attr(w.slot());
      v2f pj[NPAIR], z[NPAIR];
      lds_row<COL>(lds + w.row() * RS, pj);
      deg += 1.f;
      edge_preact(wa, a, Pi, pj, z);
#pragma unroll
      for (int p = 0; p < NPAIR; ++p) S[p] += __builtin_elementwise_max(z[p], splat(0.f));
    }
  return deg;
}


// ---- relu folded into the last fma of an edge pre-activation -----------------------------------------------------
// v_max_f32 is not packed on gfx950, so  S += relu(z)  costs two v_max + one v_pk_add per output pair -- 10 of the 35
// VALU slots of one edge direction.  The VOP3P clamp bit clamps a result to [0, 1] for free; computing the
// pre-activation SCALED by 2^-40 (every term times a power of two: bit-exact, fp32 rounding commutes with it unless a
// value underflows below 2^-126, i.e. |z| < 2^-86) turns relu(z) = 2^40 clamp(2^-40 z) for every |z| < 2^40 ~ 1e12.
// NaN clamps to 0, as v_max(NaN, 0) did.  The attr values a0, a1, a2 are broadcast from the halves of two register
// pairs with op_sel (the compiler would spend six v_mov per slot on duplicating them).
#define RELU_SCALE 9.094947017729282e-13f   // 2^-40
#define RELU_UNSCALE 1099511627776.f        // 2^40
__device__ __forceinline__ v2f pk_fma_lo(v2f w, v2f a, v2f z) {  // z + w * (a.x, a.x)
  v2f r;
  asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[1,0,1]" : "=v"(r) : "s"(w), "v"(a), "v"(z));
  return r;
}
__device__ __forceinline__ v2f pk_fma_hi(v2f w, v2f a, v2f z) {  // z + w * (a.y, a.y)
  v2f r;
  asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[0,1,0] op_sel_hi:[1,1,1]" : "=v"(r) : "s"(w), "v"(a), "v"(z));
  return r;
}
__device__ __forceinline__ v2f pk_fma_lo_clamp(v2f w, v2f a, v2f z) {  // clamp(z + w * (a.x, a.x), 0, 1)
  v2f r;
  asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[1,0,1] clamp" : "=v"(r) : "s"(w), "v"(a), "v"(z));
  return r;
}

// One 16-byte slot record.  STREAM: requested with the non-temporal policy (global_load_dwordx4 ... nt).  The fused dirichlet Broyden
// step asks for it: its records are read once per iteration with the whole history streamed in between -- 69.8 -> 66.7 us per step
// at 1M nodes (profiles/stream_policy_ab.txt).  Back-to-back plain f, whose records stay in the Infinity Cache, lost 5 - 8 % with it
// (50.2 -> 52.5 - 54 us) and keeps the default policy, as does every other kernel that walks the slots.
template <bool STREAM>
__device__ __forceinline__ uint4 ld_slot(const uint4* __restrict__ p) {
  if constexpr (STREAM) {
    typedef unsigned u32x4s __attribute__((ext_vector_type(4)));
    const u32x4s t = __builtin_nontemporal_load(reinterpret_cast<const u32x4s*>(p));
    return make_uint4(t.x, t.y, t.z, t.w);
  } else {
    return *p;
  }
}

// Both directions of the neighbour sum in ONE walk over the slots: a pair-merged slot is decoded once, its 80-byte (8 D) LDS row
// [to | from] is read once, and the IN half (Phi_to, mirrored attr weights) and the OUT half (Phi_from) are evaluated back
// to back.  Needs both attr blocks (6 D = 60 wave-uniform floats) in SGPRs for the whole loop -- affordable once the phase
// barriers keep every other scalar load out of the loop's live range.  S_to / S_fr come back UNSCALED (multiplied by 2^40
// at the end).  Slot records are loaded one round ahead; two rounds ahead was measured and removed (profiles/r2_f_tile_ab_runs.txt:
// plain f 61.0 - 62.6 vs 57.5 - 58.8 us).
template <int RS, bool STREAM = false>
__device__ __forceinline__ void edge_pass_both_clamp(const uint4* __restrict__ slots, int nslots, const float* __restrict__ lds,
                                                     const float* __restrict__ AT_to, const float* __restrict__ AT_fr,
                                                     const v2f* Pi_to, const v2f* Pi_fr, v2f* S_to, v2f* S_fr,
                                                     float& deg_in, float& deg_out) {
  v2f wt[3 * NPAIR], wf[3 * NPAIR], pt[NPAIR], pf[NPAIR];
#pragma unroll
  for (int i = 0; i < 3 * NPAIR; ++i) {
    wt[i] = reinterpret_cast<const v2f*>(AT_to)[i];
    wf[i] = reinterpret_cast<const v2f*>(AT_fr)[i];
  }
  const v2f sc = splat(RELU_SCALE);
#pragma unroll
  for (int p = 0; p < NPAIR; ++p) {
    pt[p] = Pi_to[p] * sc;
    pf[p] = Pi_fr[p] * sc;
  }
  deg_in = deg_out = 0.f;
  if (nslots <= 0) return;
  uint4 c0 = ld_slot<STREAM>(slots);
  for (int r = 0; r < nslots; ++r) {
    const uint4 nx = ld_slot<STREAM>(slots + (int64_t)min(r + 1, nslots - 1) * 64);
    const unsigned w = c0.x;
    if ((w & 0xFFFFu) != ELL_EMPTY) {
      const v2f a01 = (v2f){__uint_as_float(c0.y), __uint_as_float(c0.z)} * sc;
      const v2f a2 = (v2f){__uint_as_float(c0.w) * RELU_SCALE, 0.f};
      const float4* row = reinterpret_cast<const float4*>(lds + (int)(w & 0xFFFFu) * RS);
      float4 v[NPAIR];   // [to D | from D] = NPAIR quads
#pragma unroll
      for (int q = 0; q < NPAIR; ++q) v[q] = row[q];
      if (w & SLOT_IN) {
        v2f z[NPAIR];
#pragma unroll
        for (int p = 0; p < NPAIR; ++p) z[p] = quad_pair(v, p);
        deg_in += 1.f;
#pragma unroll
        for (int p = 0; p < NPAIR; ++p) z[p] = __builtin_elementwise_fma(z[p], sc, pt[p]);
#pragma unroll
        for (int p = 0; p < NPAIR; ++p) z[p] = pk_fma_lo(wt[p], a01, z[p]);
#pragma unroll
        for (int p = 0; p < NPAIR; ++p) z[p] = pk_fma_hi(wt[NPAIR + p], a01, z[p]);
#pragma unroll
        for (int p = 0; p < NPAIR; ++p) z[p] = pk_fma_lo_clamp(wt[2 * NPAIR + p], a2, z[p]);
#pragma unroll
        for (int p = 0; p < NPAIR; ++p) S_to[p] += z[p];
      }
      if (w & SLOT_OUT) {
        v2f z[NPAIR];
#pragma unroll
        for (int p = 0; p < NPAIR; ++p) z[p] = quad_pair(v, NPAIR + p);
        deg_out += 1.f;
#pragma unroll
        for (int p = 0; p < NPAIR; ++p) z[p] = __builtin_elementwise_fma(z[p], sc, pf[p]);
#pragma unroll
        for (int p = 0; p < NPAIR; ++p) z[p] = pk_fma_lo(wf[p], a01, z[p]);
#pragma unroll
        for (int p = 0; p < NPAIR; ++p) z[p] = pk_fma_hi(wf[NPAIR + p], a01, z[p]);
#pragma unroll
        for (int p = 0; p < NPAIR; ++p) z[p] = pk_fma_lo_clamp(wf[2 * NPAIR + p], a2, z[p]);
#pragma unroll
        for (int p = 0; p < NPAIR; ++p) S_fr[p] += z[p];
      }
    }
    c0 = nx;
  }
  const v2f us = splat(RELU_UNSCALE);
#pragma unroll
  for (int p = 0; p < NPAIR; ++p) {
    S_to[p] *= us;
    S_fr[p] *= us;
  }
}
