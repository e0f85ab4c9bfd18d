// What the float64 reference path shares (gfx950): the weight layout, the map handle and the family dispatch of fgnn_f64.hip /
// fgnn_f64_deriv.hip (their arithmetic is f64_node.h's), and the block shape and fixed-order reductions of solver_f64.hip,
// krylov_f64.hip and poisson_cg.hip.  Included by those five, by f64_node.h and by nothing else.
#pragma once
#include "common.h"
#include "internal.h"

#if PSIGNN_D != 10
#error "the float64 reference path is part of the default-width library only"
#endif

// ---------------------------------------------------------------------------------------------
// Weight layout (doubles): the deqdss.f.* tensors of the state dict, each nn.Linear (out, in) row-major, in this order
//   laynorm.weight[10] laynorm.bias[10] alpha.0.weight[30+P] alpha.0.bias[1]
//   per layer l: phi_to_list.l.mlp.mlp.{0.weight[10x23] 0.bias[10] 2.weight[10x10] 2.bias[10]}  phi_from_list.l.mlp.mlp.{same}
//                update_list.l.mlp.{0.weight[10x(30+P)] 0.bias[10] 2.weight[10x10] 2.bias[10]}
//   mixed only:  phi_neumann.mlp.mlp.{0.weight[10x23] 0.bias 2.weight 2.bias}  update_neumann.mlp.{0.weight[10x(22+P)] 0.bias 2.weight 2.bias}
// P = 2 (dirichlet) / 3 (mixed).  No padding, nothing derived.
// ---------------------------------------------------------------------------------------------
template <int P>
struct W64 {
  static constexpr int CAT = 3 * D + P, EIN = 2 * D + 3, NCAT = 2 * D + P + 2;
  static constexpr int LN_G = 0, LN_B = D, AL_W = 2 * D, AL_B = 2 * D + CAT, SHARED = 2 * D + CAT + 1;
  static constexpr int PHI_W1 = 0, PHI_B1 = D * EIN, PHI_W2 = D * EIN + D, PHI_B2 = D * EIN + D + D * D, PHI_SZ = D * EIN + 2 * D + D * D;
  static constexpr int UPD_B1 = D * CAT, UPD_W2 = D * CAT + D, UPD_B2 = D * CAT + D + D * D, UPD_SZ = D * CAT + 2 * D + D * D;
  static constexpr int NEU_B1 = D * NCAT, NEU_W2 = D * NCAT + D, NEU_B2 = D * NCAT + D + D * D, NEU_SZ = D * NCAT + 2 * D + D * D;
  static constexpr int LAYER = 2 * PHI_SZ + UPD_SZ;
  __host__ __device__ static constexpr int layer(int l) { return SHARED + l * LAYER; }
  __host__ __device__ static constexpr int total(int nl, bool mixed) { return SHARED + nl * LAYER + (mixed ? PHI_SZ + NEU_SZ : 0); }
};
static_assert(W64<2>::total(1, false) == 1193 && W64<3>::total(1, true) == 1924, "float64 weight layout at D = 10");

struct psignn_f64 {
  const psignn_plan* p = nullptr;   // borrowed: the plan outlives the handle
  double *csr_attr = nullptr, *csc_attr = nullptr;   // (Ep, 3) each, in the order of the plan's csr_nbr / csc_nbr
  double* pp[2] = {nullptr, nullptr};                // layer ping-pong of a multi-layer dirichlet block, made on first use
};
// both edge lists and the node flags of a map handle, in the order every layer kernel takes them
#define F64_EDGES(f) (f)->p->csr_ptr, (f)->p->csr_nbr, (f)->csr_attr, (f)->p->csc_ptr, (f)->p->csc_nbr, (f)->csc_attr, (f)->p->flags
// The family of a plan: runs the statements with P, MIXED and L = W64<P> of a mixed plan (<3, true>) or a dirichlet one (<2, false>),
// so that every launch picks its instantiation and the matching L::layer(l) / L::layer(nl) offsets in one place.
#define F64_FAMILY(mixed, ...)                        \
  do {                                                \
    if (mixed) {                                      \
      [[maybe_unused]] constexpr int P = 3;           \
      [[maybe_unused]] constexpr bool MIXED = true;   \
      using L [[maybe_unused]] = W64<3>;              \
      __VA_ARGS__;                                    \
    } else {                                          \
      [[maybe_unused]] constexpr int P = 2;           \
      [[maybe_unused]] constexpr bool MIXED = false;  \
      using L [[maybe_unused]] = W64<2>;              \
      __VA_ARGS__;                                    \
    }                                                 \
  } while (0)

#define F64_TB 256       // threads per block of the vector and reduction kernels: four waves, one partial per block
#define F64_CHUNK 1024   // elements of a dots chunk: 8 x (64 lanes x 2 doubles)

// ------------------------------------------------------------------ reductions (fixed shape, fixed order; no floating-point atomics)
__device__ __forceinline__ double f64_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;   // lane 0 holds the sum
}
__device__ __forceinline__ double f64_block_sum(double v, double* sh /* 4 */) {
  v = f64_wave_sum(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  const double s = (sh[0] + sh[1]) + (sh[2] + sh[3]);
  __syncthreads();
  return s;
}
__device__ __forceinline__ double f64_block_max(double v, double* sh /* 4 */) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_down(v, o, 64));
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  const double s = fmax(fmax(sh[0], sh[1]), fmax(sh[2], sh[3]));
  __syncthreads();
  return s;
}
// one block: the n block partials, each thread its stride in ascending order, then the block sum
__device__ __forceinline__ double f64_final_sum(const double* __restrict__ part, int64_t n, double* sh) {
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += F64_TB) s += part[i];
  return f64_block_sum(s, sh);
}
// 16 bytes of a chunk.  A lane past the end of the last chunk reads the chunk's first element (always inside) and drops the value.
template <bool FULL>
__device__ __forceinline__ double2 f64_ld2(const double* __restrict__ p, int64_t e, int64_t base, int64_t M) {
  if (FULL) return *(const double2*)(p + e);
  const bool in = e < M;
  const double2 v = *(const double2*)(p + (in ? e : base));
  double2 r;
  r.x = in ? v.x : 0.0;
  r.y = in ? v.y : 0.0;
  return r;
}
