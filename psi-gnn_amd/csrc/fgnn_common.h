// Small per-lane helpers shared by the GNN-block kernels (gfx950).
#pragma once
#include "common.h"

// one latent row (D floats, 8-byte aligned) as D/2 float2.  load10 / store10: the same under the names the width-10-only
// translation units were written with.
__device__ __forceinline__ void loadD(const float* __restrict__ p, float* __restrict__ r) {
  const float2* q = reinterpret_cast<const float2*>(p);
#pragma unroll
  for (int i = 0; i < NPAIR; ++i) {
    float2 t = q[i];
    r[2 * i] = t.x;
    r[2 * i + 1] = t.y;
  }
}
__device__ __forceinline__ void storeD(float* __restrict__ p, const float* __restrict__ r) {
  float2* q = reinterpret_cast<float2*>(p);
#pragma unroll
  for (int i = 0; i < NPAIR; ++i) q[i] = make_float2(r[2 * i], r[2 * i + 1]);
}
__device__ __forceinline__ void load10(const float* __restrict__ p, float* __restrict__ r) { loadD(p, r); }
__device__ __forceinline__ void store10(float* __restrict__ p, const float* __restrict__ r) { storeD(p, r); }

// out[o] (+)= sum_k W[o*ld + off + k] * x[k],  o < D, k < K   (W wave-uniform -> scalar loads)
template <int K, bool ACC>
__device__ __forceinline__ void matvecD(const float* __restrict__ W, int ld, int off, const float* x, float* out) {
#pragma unroll
  for (int o = 0; o < D; ++o) {
    float s = ACC ? out[o] : 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) s = fmaf(W[o * ld + off + k], x[k], s);
    out[o] = s;
  }
}

template <int K, bool ACC>
__device__ __forceinline__ void matvec10(const float* __restrict__ W, int ld, int off, const float* x, float* out) {
  matvecD<K, ACC>(W, ld, off, x, out);
}

// Compiler-level memory barrier between the phases of a kernel.  The node kernels read > 1 000 wave-uniform weights; fully
// unrolled, the compiler hoists all their scalar loads to the top and then spills hundreds of SGPRs into VGPR lanes
// (v_writelane / v_readlane = VALU issue slots; in the record-writing instantiation of the mixed gather VJP that went wrong on
// ROCm 7.2: per-lane values came back as spilled weights).  The barrier keeps each phase's scalar loads next to their use.
#define PHASE() asm volatile("" ::: "memory")

// out[k] (+)= sum_o W[o*ld + off + k] * g[o]   (transposed product, W wave-uniform)
template <int K, bool ACC>
__device__ __forceinline__ void matvecT(const float* __restrict__ W, int ld, int off, const float* g, float* out) {
#pragma unroll
  for (int k = 0; k < K; ++k) {
    float s = ACC ? out[k] : 0.f;
#pragma unroll
    for (int o = 0; o < D; ++o) s = fmaf(W[o * ld + off + k], g[o], s);
    out[k] = s;
  }
}

// z[o] = Pi[o] + pj[o] + W1[o, 2D:2D+3] . a   (pre-activation of one edge; W1 = first Phi layer, row length 2 D + 3)
__device__ __forceinline__ void edge_z(const float* __restrict__ W1, const float* Pi, const float* pj, float a0, float a1,
                                       float a2, float* z) {
  constexpr int EIN = 2 * D + 3;
#pragma unroll
  for (int o = 0; o < D; ++o) {
    float t = Pi[o] + pj[o];
    t = fmaf(W1[o * EIN + 2 * D], a0, t);
    t = fmaf(W1[o * EIN + 2 * D + 1], a1, t);
    t = fmaf(W1[o * EIN + 2 * D + 2], a2, t);
    z[o] = t;
  }
}

// ---- parameter-gradient records (ws::REC_F / ws::REC_X floats per node, reduced by fgnn_pgrad.hip): 16-float groups
// one group: v[0..n) then up to five trailing values, rest 0
__device__ __forceinline__ void rec_group(float* __restrict__ g, const float* v, int n, float t0 = 0.f, float t1 = 0.f,
                                          float t2 = 0.f, float t3 = 0.f, float t4 = 0.f) {
  float r[16];
#pragma unroll
  for (int i = 0; i < 16; ++i)
    r[i] = i < n ? v[i] : (i == n ? t0 : (i == n + 1 ? t1 : (i == n + 2 ? t2 : (i == n + 3 ? t3 : (i == n + 4 ? t4 : 0.f)))));
  float4* q = reinterpret_cast<float4*>(g);
#pragma unroll
  for (int i = 0; i < 4; ++i) q[i] = make_float4(r[4 * i], r[4 * i + 1], r[4 * i + 2], r[4 * i + 3]);
}
__device__ __forceinline__ void rec_zero(float* __restrict__ g, int first, int last) {  // groups [first, last)
  for (int i = first * 4; i < last * 4; ++i) reinterpret_cast<float4*>(g)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
}
