// GMRES on the device for the Newton-Krylov solver (gfx950): Arnoldi with classical Gram-Schmidt applied twice, the
// Hessenberg least-squares problem by Givens rotations, the solution update -- vector sweeps on the same coalesced float4
// kernels as the Broyden solver, the small dense part in one block, nothing on the host but the launch sequence.
//
// Reference: none executable -- dirichlet/psignn/utilities/solver.py:6 imports scipy.optimize.newton_krylov and never calls
// it; BASELINE configs[4] names the Newton-Krylov / JVP path.  The operator is applied by the caller
// (the analytic JVP kernel of the GNN block, csrc/fgnn_tile_jvp.hip): per Arnoldi step it writes A v_j's raw product
// J v_j into basis slot j + 1 and calls psignn_gmres_step, which turns it into the next basis vector:
//   dots pass 1 : w = J v_j (the raw product; the shift enters the Hessenberg's diagonal in `finish`: the Krylov spaces of J and
//                 of J - shift I are the same, and orthogonalising J v_j instead of J v_j - v_j keeps the big -v_j component --
//                 pure cancellation against the basis -- out of the Gram-Schmidt passes), h_i = <v_i, w>, i <= j  (basis read once)
//   axpy pass 1 : w -= sum_i h_i v_i                                                (basis read once)
//   dots pass 2 / axpy pass 2 : the same again on the result ("twice is enough"), with the partials of |w|^2 -- run only when
//                 the first pass cancelled: |w'|^2 < 1/2 |w|^2 (the Daniel-Gragg-Kaufman-Stewart criterion, decided on the
//                 device by k_gm_decide; PSIGNN_GMRES_REORTH=always restores the unconditional second pass)
//   finish      : H[:, j] = h1 + h2 - shift e_j, H[j+1, j] = |w|; previous rotations applied, new rotation, residual |g_{j+1}|;
//                 stop flag when |g_{j+1}| <= eta * beta
//   scale       : v_{j+1} = w / |w|
// = 2 (j + 1) + O(1) vector passes per step, 4 (j + 1) when the second pass runs.  Reductions: fixed-shape partial sums in a fixed order (reproducible).
#include "vec_helpers.h"
#include "internal.h"
#include "solver_shapes.h"
#include "gmres_dense.h"
#include <algorithm>
#include <stddef.h>
#include <vector>
#include <stdlib.h>
#include <string.h>

struct GmresState {
  int32_t k;          // Arnoldi steps completed
  int32_t done;       // the relative linear residual reached eta (or a breakdown: |w| == 0)
  int32_t breakdown;
  int32_t reorth;     // this step's second Gram-Schmidt pass runs (k_gm_decide)
  double beta;        // |b|
  double resid;       // current |g_{k}| (absolute residual of the least-squares problem)
  double hn;          // |w| of the last step
  double n0sq;        // |w|^2 before the first pass of the current step
  int32_t n_reorth;   // steps of this solve that needed the second pass
  int32_t pad;
};

struct psignn_gmres {
  int64_t M = 0, ld = 0;
  int m = 0;
  int vec = 16, nblk = 0, npart = 0;
  float* V = nullptr;        // caller-owned basis: (m + 1, ld)
  float* part = nullptr;     // (nblk, ldp) dot partials: one value per block and basis vector, vectors contiguous
  int ldp = 0;               // m + 2 rounded up to 64
  float* coef = nullptr;     // (m + 2) coefficients of the current pass (float, like the vectors)
  double* H = nullptr;       // (m + 1, m) column-major: R after the rotations (column j has j + 1 entries) | raw h in work
  double *cs = nullptr, *sn = nullptr, *g = nullptr, *hcol = nullptr, *y = nullptr, *res_hist = nullptr;
  GmresState* st = nullptr;
  GmresState* h_st = nullptr;
  size_t bytes = 0;
  // restarted solve of the adjoint system (end of this file): solve-level state and per-cycle traces, allocated by the first such solve
  struct AdjState* ast = nullptr;
  struct AdjState* h_ast = nullptr;
  double *a_rel = nullptr, *a_abs = nullptr;
  int a_cap = 0;             // entries of each trace
  // augmented restarts of the adjoint solve (psignn_gmres_create_aug)
  int augment = 0;           // corrections a solve on this handle may keep
  float* Z = nullptr;        // caller-owned ring of corrections: (augment + 1, ld); NULL when augment = 0
};

// Solve-level state of the restarted adjoint solve (one per handle, device memory; GmresState above is re-armed every cycle)
struct AdjState {
  int32_t cycles;       // restart cycles begun = entries of the traces
  int32_t products;     // transposed products spent: Arnoldi steps that ran + one per cycle after the first
  int32_t done;         // the solve is over (GmresState::done is raised with it: every gated kernel then returns)
  int32_t stop;         // 0 budget, 1 tolerance, 2 stagnation
  int32_t steps_left;   // Arnoldi steps this cycle may take (<= m; the budget keeps one product for the next cycle's residual)
  int32_t improved;     // this cycle's iterate has the lowest rel so far: k_ag_keep copies it
  int32_t n_reorth;     // copy of GmresState::n_reorth at the last check
  int32_t pad;
  double prev_rel, lowest, lowest_abs;
  double rnorm;         // |r| of this cycle (row 0 is divided by it)
  // augmented restarts (cleared by k_lg_init, written by k_lg_check / k_lg_norm; a solve without options touches none of them)
  int32_t nk, ka;       // this cycle's plan: Krylov steps, augmentation steps (nk + ka = steps_left)
  int32_t stored;       // corrections in the ring
  int32_t head;         // the ring slot that is due
  int32_t n_aug;        // augmentation steps of this solve
  int32_t dy_ok;        // the last cycle's correction went into the ring (its slot still holds dy, not dy / |dy|)
  double dyn;           // |dy| of the last cycle
};

// (every kernel of the restarted adjoint solve keeps its code in a *_body function: the single-handle kernel and its batched form,
// one launch for the replicas of a shard at the end of this file, both call it)
// (bd, gd: the launch's blockDim.x and gridDim.x, read by the kernel -- inside a device function the compiler lowers blockDim.x to
// its form for non-uniform work-groups)
__device__ __forceinline__ void gm_init_body(GmresState* st, double* g, double* res_hist, int m, unsigned bd, unsigned gd) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    st->k = 0; st->done = 0; st->breakdown = 0; st->reorth = 1; st->pad = 0; st->beta = 0.0; st->resid = 0.0; st->hn = 0.0;
    st->n0sq = 0.0; st->n_reorth = 0;
  }
  for (int i = blockIdx.x * bd + threadIdx.x; i <= m + 1; i += gd * bd) {
    g[i] = 0.0;
    res_hist[i] = 0.0;
  }
}
__global__ void k_gm_init(GmresState* st, double* g, double* res_hist, int m) {
  gm_init_body(st, g, res_hist, m, blockDim.x, gridDim.x);
}

// partials of <a, a> (one per block): part[blockIdx.x]
template <int VEC>
__global__ __launch_bounds__(TB) void k_gm_norm2(int64_t M, const float* __restrict__ a, float* __restrict__ part, int npart) {
  int64_t e0 = elem0<VEC>();
  float s = 0.f, z = 0.f;
  if (e0 < M) {
    float x[VEC];
    ldv<VEC>(a, e0, M, x);
#pragma unroll
    for (int i = 0; i < VEC; ++i) s = fmaf(x[i], x[i], s);
  }
  block_pair_store(s, z, part, npart);
}

// beta = |b| ; g[0] = beta ; resid = beta
__global__ __launch_bounds__(TB) void k_gm_begin(GmresState* st, const float* __restrict__ part, int nblk, double* __restrict__ g,
                                                 double* __restrict__ res_hist) {
  __shared__ double sh[TB];
  const double s = block_sum_partials(part, nblk, sh);
  if (threadIdx.x == 0) {
    const double beta = (double)(float)sqrt(s);
    st->beta = beta;
    st->resid = beta;
    g[0] = beta;
    res_hist[0] = beta;
    if (!(beta > 0.0)) {   // zero right-hand side: nothing to solve
      st->done = 1;
      st->breakdown = 1;
    }
  }
}

// dst = src * (1 / scale), scale = sqrt of a device double (beta or hn)
template <int VEC>
__device__ __forceinline__ void gm_scale_body(int64_t M, const float* __restrict__ src, float* __restrict__ dst,
                                              const double* __restrict__ scale, const GmresState* __restrict__ st, int gate) {
  if (gate && st->done) return;
  int64_t e0 = elem0<VEC>();
  if (e0 >= M) return;
  const float inv = 1.f / (float)(*scale);
  float x[VEC];
  ldv<VEC>(src, e0, M, x);
#pragma unroll
  for (int i = 0; i < VEC; ++i) x[i] *= inv;
  stv<VEC>(dst, e0, M, x);
}
template <int VEC>
__global__ __launch_bounds__(TB) void k_gm_scale(int64_t M, const float* __restrict__ src, float* __restrict__ dst,
                                                 const double* __restrict__ scale, const GmresState* __restrict__ st, int gate) {
  gm_scale_body<VEC>(M, src, dst, scale, st, gate);
}

// dots pass: optional first transform w <- w - shift * v_j (stored back); per-BLOCK partials of <v_i, w>, i <= j, written as
// coalesced rows part[block * ldp + i] (vec_helpers.h PairStash: round 2's one 4-byte store per wave and basis vector cost the
// sweep 8 % of its rate).  pass 0 also leaves the partials of |w|^2 in column j + 1; pass 1 returns at once unless st->reorth
template <int VEC>
__device__ __forceinline__ void gm_dots_body(int64_t M, int64_t ld, int j, float shift, const GmresState* __restrict__ st,
                                             const float* __restrict__ V, float* __restrict__ w, float* __restrict__ part,
                                             int ldp, int pass) {
  __shared__ PairStash<1> sh;
  if (st->done || (pass && !st->reorth)) return;
  int64_t e0 = elem0<VEC>();
  const bool act = e0 < M;
  float x[VEC];
  if (act) {
    ldv<VEC>(w, e0, M, x);
    if (shift != 0.f) {
      float v[VEC];
      ldv<VEC>(V + (int64_t)j * ld, e0, M, v);
#pragma unroll
      for (int i = 0; i < VEC; ++i) x[i] = fmaf(-shift, v[i], x[i]);
      stv<VEC>(w, e0, M, x);
    }
  } else {
#pragma unroll
    for (int i = 0; i < VEC; ++i) x[i] = 0.f;
  }
  const int wv = threadIdx.x >> 6;
  const bool lead = (threadIdx.x & 63) == 0;
  float* rowb = part + (int64_t)blockIdx.x * ldp;
  const int last = pass == 0 ? j + 1 : j;     // columns 0 .. last: the j + 1 dot products (+ |w|^2 in pass 0)
  for (int i = 0; i <= last; ++i) {
    float s = 0.f;
    if (i <= j) {
      if (act) {
        float v[VEC];
        ldv<VEC>(V + (int64_t)i * ld, e0, M, v);
#pragma unroll
        for (int c = 0; c < VEC; ++c) s = fmaf(v[c], x[c], s);
      }
    } else {
#pragma unroll
      for (int c = 0; c < VEC; ++c) s = fmaf(x[c], x[c], s);
    }
    s = wave_sum(s);
    const int q = i & 63;
    if (lead) sh.v[0][wv][q] = s;
    if (q == 63 || i == last) {
      float* const rows[1] = {rowb + (i - q)};
      stash_flush<1>(sh, q + 1, rows);
    }
  }
}
template <int VEC>
__global__ __launch_bounds__(TB) void k_gm_dots(int64_t M, int64_t ld, int j, float shift, const GmresState* __restrict__ st,
                                                const float* __restrict__ V, float* __restrict__ w, float* __restrict__ part,
                                                int ldp, int pass) {
  gm_dots_body<VEC>(M, ld, j, shift, st, V, w, part, ldp, pass);
}

// one block per coefficient: coef[i] = sum over the blocks of column i of the partials (rounded to float like the vectors they scale)
// (pass 0: one more block, i = n_coef, sums the |w|^2 column into st->n0sq)
__device__ __forceinline__ void gm_reduce_body(GmresState* __restrict__ st, const float* __restrict__ part, int nrows, int ldp,
                                               float* __restrict__ coef, double* __restrict__ hcol, int accumulate, int n_coef) {
  __shared__ double sh[TB];
  if (st->done || (accumulate && !st->reorth)) return;
  const int i = blockIdx.x;
  const double s = block_sum_col(part + i, nrows, ldp, sh);
  if (i == n_coef) {
    if (threadIdx.x == 0) st->n0sq = s;
    return;
  }
  if (threadIdx.x == 0) {
    const float c = (float)s;
    coef[i] = c;
    hcol[i] = accumulate ? hcol[i] + (double)c : (double)c;
  }
}
__global__ __launch_bounds__(TB) void k_gm_reduce(GmresState* __restrict__ st, const float* __restrict__ part, int nrows, int ldp,
                                                  float* __restrict__ coef, double* __restrict__ hcol, int accumulate, int n_coef) {
  gm_reduce_body(st, part, nrows, ldp, coef, hcol, accumulate, n_coef);
}

// axpy pass: w -= sum_{i <= j} coef[i] v_i ; partials of |w|^2 (one per block)
template <int VEC>
__device__ __forceinline__ void gm_axpy_body(int64_t M, int64_t ld, int j, const GmresState* __restrict__ st,
                                             const float* __restrict__ V, float* __restrict__ w,
                                             const float* __restrict__ coef, float* __restrict__ npartial, int nblk, int pass) {
  if (st->done || (pass && !st->reorth)) return;
  int64_t e0 = elem0<VEC>();
  float s = 0.f, z = 0.f;
  if (e0 < M) {
    float x[VEC];
    ldv<VEC>(w, e0, M, x);
    for (int i = 0; i <= j; ++i) {
      const float c = coef[i];
      float v[VEC];
      ldv<VEC>(V + (int64_t)i * ld, e0, M, v);
#pragma unroll
      for (int q = 0; q < VEC; ++q) x[q] = fmaf(-c, v[q], x[q]);
    }
    stv<VEC>(w, e0, M, x);
#pragma unroll
    for (int q = 0; q < VEC; ++q) s = fmaf(x[q], x[q], s);
  }
  block_pair_store(s, z, npartial, nblk);
}
template <int VEC>
__global__ __launch_bounds__(TB) void k_gm_axpy(int64_t M, int64_t ld, int j, const GmresState* __restrict__ st,
                                                const float* __restrict__ V, float* __restrict__ w,
                                                const float* __restrict__ coef, float* __restrict__ npartial, int nblk, int pass) {
  gm_axpy_body<VEC>(M, ld, j, st, V, w, coef, npartial, nblk, pass);
}

// One block, between the passes: does the first pass's result need the second one?  |w'|^2 < 1/2 |w|^2 (DGKS); `always` != 0: yes.
__device__ __forceinline__ void gm_decide_body(GmresState* st, const float* __restrict__ npartial, int nblk, int always) {
  __shared__ double sh[TB];
  if (st->done) return;
  const double n1sq = block_sum_partials(npartial, nblk, sh);
  if (threadIdx.x == 0) {
    const int r = always || !(n1sq >= 0.5 * st->n0sq);   // (NaN -> reorthogonalise)
    st->reorth = r;
    st->n_reorth += r;
  }
}
__global__ __launch_bounds__(TB) void k_gm_decide(GmresState* st, const float* __restrict__ npartial, int nblk, int always) {
  gm_decide_body(st, npartial, nblk, always);
}

// One block: finish column j of the Hessenberg matrix and the least-squares update.
__device__ __forceinline__ void gm_finish_body(GmresState* st, const float* __restrict__ npartial, int nblk, int j, int m,
                                               double* __restrict__ H, double* __restrict__ cs, double* __restrict__ sn,
                                               double* __restrict__ g, const double* __restrict__ hcol,
                                               double* __restrict__ res_hist, double eta, double shift,
                                               const int32_t* __restrict__ limit) {
  __shared__ double sh[TB];
  if (st->done) return;
  const double s2 = block_sum_partials(npartial, nblk, sh);
  if (threadIdx.x != 0) return;
  const double hn = (double)(float)sqrt(s2);
  st->hn = hn;
  double* col = H + (int64_t)j * (m + 1);
  for (int i = 0; i <= j; ++i) col[i] = hcol[i];
  col[j] -= shift;   // Hessenberg of J - shift I from the Arnoldi relation of J
  col[j + 1] = hn;
  for (int i = 0; i < j; ++i) {   // previous rotations
    const double t = cs[i] * col[i] + sn[i] * col[i + 1];
    col[i + 1] = -sn[i] * col[i] + cs[i] * col[i + 1];
    col[i] = t;
  }
  const double a = col[j], b = col[j + 1];
  const double r = sqrt(a * a + b * b);
  const double c = r > 0.0 ? a / r : 1.0, s = r > 0.0 ? b / r : 0.0;
  cs[j] = c;
  sn[j] = s;
  col[j] = r;
  col[j + 1] = 0.0;
  g[j + 1] = -s * g[j];
  g[j] = c * g[j];
  const double resid = fabs(g[j + 1]);
  st->resid = resid;
  st->k = j + 1;
  res_hist[j + 1] = resid;
  if (resid <= eta * st->beta) st->done = 1;
  if (limit && j + 1 >= *limit) st->done = 1;   // the adjoint solve's per-cycle step allowance (a device value; NULL: none)
  if (!(hn > 0.0)) {   // lucky breakdown: the Krylov space is invariant, the least-squares solution is exact
    st->done = 1;
    st->breakdown = 1;
  }
}
__global__ __launch_bounds__(TB) void k_gm_finish(GmresState* st, const float* __restrict__ npartial, int nblk, int j, int m,
                                                  double* __restrict__ H, double* __restrict__ cs, double* __restrict__ sn,
                                                  double* __restrict__ g, const double* __restrict__ hcol,
                                                  double* __restrict__ res_hist, double eta, double shift,
                                                  const int32_t* __restrict__ limit) {
  gm_finish_body(st, npartial, nblk, j, m, H, cs, sn, g, hcol, res_hist, eta, shift, limit);
}

// One block: y = R^{-1} g for the first k columns
__device__ __forceinline__ void gm_backsolve_body(const GmresState* __restrict__ st, int k_override, int m, const double* __restrict__ H,
                                                  const double* __restrict__ g, double* __restrict__ y, float* __restrict__ coef) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const int k = k_override > 0 ? min(k_override, st->k) : st->k;
  for (int i = k - 1; i >= 0; --i) {
    double s = g[i];
    for (int q = i + 1; q < k; ++q) s -= H[(int64_t)q * (m + 1) + i] * y[q];
    const double d = H[(int64_t)i * (m + 1) + i];
    y[i] = d != 0.0 ? s / d : 0.0;
  }
  for (int i = 0; i < k; ++i) coef[i] = (float)y[i];
  for (int i = k; i <= m; ++i) coef[i] = 0.f;
}
__global__ void k_gm_backsolve(const GmresState* __restrict__ st, int k_override, int m, const double* __restrict__ H,
                               const double* __restrict__ g, double* __restrict__ y, float* __restrict__ coef) {
  gm_backsolve_body(st, k_override, m, H, g, y, coef);
}

// dst = base + scale * sum_{i < k} coef[i] v_i   (base may be NULL: dst = the combination)
template <int VEC>
__device__ __forceinline__ void gm_combine_body(int64_t M, int64_t ld, const GmresState* __restrict__ st, int k_override,
                                                const float* __restrict__ V, const float* __restrict__ coef,
                                                const float* __restrict__ base, float scale, float* __restrict__ dst) {
  int64_t e0 = elem0<VEC>();
  if (e0 >= M) return;
  const int k = k_override > 0 ? min(k_override, st->k) : st->k;
  float acc[VEC];
#pragma unroll
  for (int q = 0; q < VEC; ++q) acc[q] = 0.f;
  for (int i = 0; i < k; ++i) {
    const float c = coef[i];
    float v[VEC];
    ldv<VEC>(V + (int64_t)i * ld, e0, M, v);
#pragma unroll
    for (int q = 0; q < VEC; ++q) acc[q] = fmaf(c, v[q], acc[q]);
  }
  if (base) {
    float b[VEC];
    ldv<VEC>(base, e0, M, b);
#pragma unroll
    for (int q = 0; q < VEC; ++q) acc[q] = fmaf(scale, acc[q], b[q]);
  } else {
#pragma unroll
    for (int q = 0; q < VEC; ++q) acc[q] *= scale;
  }
  stv<VEC>(dst, e0, M, acc);
}
template <int VEC>
__global__ __launch_bounds__(TB) void k_gm_combine(int64_t M, int64_t ld, const GmresState* __restrict__ st, int k_override,
                                                   const float* __restrict__ V, const float* __restrict__ coef,
                                                   const float* __restrict__ base, float scale, float* __restrict__ dst) {
  gm_combine_body<VEC>(M, ld, st, k_override, V, coef, base, scale, dst);
}

// g = fx - x ; partials of |g|^2 and |fx|^2 (one pair per block); optionally b = -g
template <int VEC>
__global__ __launch_bounds__(TB) void k_gm_residual(int64_t M, const float* __restrict__ x, const float* __restrict__ fx,
                                                    float* __restrict__ gout, float* __restrict__ neg_out,
                                                    float* __restrict__ part, int nblk) {
  int64_t e0 = elem0<VEC>();
  float sg = 0.f, sf = 0.f;
  if (e0 < M) {
    float a[VEC], b[VEC];
    ldv<VEC>(x, e0, M, a);
    ldv<VEC>(fx, e0, M, b);
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      sf = fmaf(b[i], b[i], sf);
      b[i] -= a[i];
      sg = fmaf(b[i], b[i], sg);
    }
    if (gout) stv<VEC>(gout, e0, M, b);
    if (neg_out) {
#pragma unroll
      for (int i = 0; i < VEC; ++i) b[i] = -b[i];
      stv<VEC>(neg_out, e0, M, b);
    }
  }
  block_pair_store(sg, sf, part, nblk);
}
__global__ __launch_bounds__(TB) void k_gm_norms_out(const float* __restrict__ part, int nblk, double* __restrict__ out2) {
  __shared__ double sh[TB];
  const double sg = block_sum_partials(part, nblk, sh);
  const double sf = block_sum_partials(part + nblk, nblk, sh);
  if (threadIdx.x == 0) {
    out2[0] = (double)(float)sqrt(sg);
    out2[1] = (double)(float)sqrt(sf);
  }
}

// ------------------------------------------------------------------------------------------ host
extern "C" void psignn_gmres_destroy(psignn_gmres_t* s) {
  if (!s) return;
  void* ptrs[] = {s->part, s->coef, s->H, s->cs, s->sn, s->g, s->hcol, s->y, s->res_hist, s->st};
  for (void* q : ptrs)
    if (q) (void)hipFree(q);
  void* aptrs[] = {s->ast, s->a_rel, s->a_abs};
  for (void* q : aptrs)
    if (q) (void)hipFree(q);
  if (s->h_st) (void)hipHostFree(s->h_st);
  if (s->h_ast) (void)hipHostFree(s->h_ast);
  delete s;
}

// width_elems: the length the vector width is chosen for (the handle's own, or the whole shard's: psignn_gmres_create_for_batch)
static int gmres_create(psignn_gmres_t** out, int64_t n_elems, int64_t ld, int m_max, float* d_basis, int64_t width_elems) {
  ARG_CHECK(out, "out is NULL");
  *out = nullptr;
  ARG_CHECK(n_elems > 0 && m_max > 0 && d_basis, "bad arguments");
  ARG_CHECK(ld >= n_elems && ld % 4 == 0, "row pitch must be >= n_elems and a multiple of 4 floats");
  psignn_gmres* s = new psignn_gmres();
  s->M = n_elems;
  s->ld = ld;
  s->m = m_max;
  s->V = d_basis;
  const shapes::VecShape v = shapes::vec_shape(n_elems, width_elems);
  s->vec = v.vec; s->nblk = v.nblk; s->npart = v.npart;
  s->ldp = (m_max + 2 + 63) / 64 * 64;
  const size_t m = (size_t)m_max;
  struct { void** p; size_t n; } allocs[] = {
      {(void**)&s->part, (size_t)s->nblk * s->ldp * 4 + 16}, {(void**)&s->coef, (m + 2) * 4 + 16},
      {(void**)&s->H, (m + 1) * (m + 1) * 8}, {(void**)&s->cs, (m + 2) * 8}, {(void**)&s->sn, (m + 2) * 8},
      {(void**)&s->g, (m + 3) * 8}, {(void**)&s->hcol, (m + 2) * 8}, {(void**)&s->y, (m + 2) * 8},
      {(void**)&s->res_hist, (m + 3) * 8}, {(void**)&s->st, sizeof(GmresState)}};
  for (auto& a : allocs) {
    if (hipMalloc(a.p, a.n) != hipSuccess) {
      psignn_set_error("gmres: hipMalloc of %zu bytes failed", a.n);
      psignn_gmres_destroy(s);
      return PSIGNN_ENOMEM;
    }
    s->bytes += a.n;
  }
  if (hipHostMalloc((void**)&s->h_st, sizeof(GmresState)) != hipSuccess) {
    psignn_set_error("gmres: hipHostMalloc failed");
    psignn_gmres_destroy(s);
    return PSIGNN_ENOMEM;
  }
  *out = s;
  return PSIGNN_OK;
}

extern "C" int psignn_gmres_create(psignn_gmres_t** out, int64_t n_elems, int64_t ld, int m_max, float* d_basis) {
  return gmres_create(out, n_elems, ld, m_max, d_basis, n_elems);
}

// A handle that will run inside psignn_gmres_solve_adjoint_lin_batch: the vector width follows the shard's length, so that all
// handles of a shard share one (as psignn_broyden_create_for_batch does for the Broyden solvers)
extern "C" int psignn_gmres_create_for_batch(psignn_gmres_t** out, int64_t n_elems, int64_t ld, int m_max, float* d_basis,
                                             int64_t shard_elems) {
  if (out) *out = nullptr;
  ARG_CHECK(shard_elems >= n_elems, "shard_elems is the sum of the shard's vector lengths: at least n_elems");
  return gmres_create(out, n_elems, ld, m_max, d_basis, shard_elems);
}

// A handle whose adjoint solves may keep up to `augment` corrections (psignn_gmres_solve_adjoint_opts): the ring is the caller's, like
// the basis, (augment + 1) rows of ld floats.  shard_elems = 0: sized for itself; otherwise psignn_gmres_create_for_batch's rule.
extern "C" int psignn_gmres_create_aug(psignn_gmres_t** out, int64_t n_elems, int64_t ld, int m_max, float* d_basis, int augment,
                                       float* d_ring, int64_t shard_elems) {
  if (out) *out = nullptr;
  ARG_CHECK(augment >= 0 && augment <= 8 && augment <= m_max - 1, "augment out of range (0 .. min(m_max - 1, 8))");
  ARG_CHECK((augment == 0) == (d_ring == nullptr), "d_ring holds (augment + 1) rows of ld floats; NULL exactly when augment is 0");
  ARG_CHECK(shard_elems == 0 || shard_elems >= n_elems, "shard_elems is 0 or the sum of the shard's vector lengths: at least n_elems");
  const int rc = gmres_create(out, n_elems, ld, m_max, d_basis, shard_elems ? shard_elems : n_elems);
  if (rc) return rc;
  (*out)->augment = augment;
  (*out)->Z = d_ring;
  return PSIGNN_OK;
}

// Device bytes the handle allocated itself (not the caller's basis): the dot partials follow the handle's blocks, hence its vector width
extern "C" size_t psignn_gmres_bytes(const psignn_gmres_t* s) { return s ? s->bytes : 0; }

// g = fx - x (d_g, may be NULL), b = -g (d_neg_g, may be NULL), h_norms[0] = |g|, h_norms[1] = |fx| (synchronous read)
extern "C" int psignn_residual_norms(psignn_gmres_t* s, const float* d_x, const float* d_fx, float* d_g, float* d_neg_g,
                                     double* h_norms, void* stream) {
  ARG_CHECK(s && d_x && d_fx && h_norms, "NULL argument");
  hipStream_t st = (hipStream_t)stream;
  VLAUNCH("k_gm_residual", st, s->vec, k_gm_residual, ((unsigned)s->nblk, TB, 0, st), s->M, d_x, d_fx, d_g, d_neg_g, s->part, s->nblk);
  k_gm_norms_out<<<1, TB, 0, st>>>(s->part, s->nblk, s->y);
  HIP_TRY(hipMemcpyAsync(h_norms, s->y, 16, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return PSIGNN_OK;
}

// Start a solve of A z = b: beta = |b|, v_0 = b / beta.
extern "C" int psignn_gmres_begin(psignn_gmres_t* s, const float* d_b, void* stream) {
  ARG_CHECK(s && d_b, "NULL argument");
  hipStream_t st = (hipStream_t)stream;
  const unsigned g = (unsigned)s->nblk;
  k_gm_init<<<4, TB, 0, st>>>(s->st, s->g, s->res_hist, s->m);
  VPLAIN(s->vec, k_gm_norm2, (g, TB, 0, st), s->M, d_b, s->part, s->nblk);
  k_gm_begin<<<1, TB, 0, st>>>(s->st, s->part, s->nblk, s->g, s->res_hist);
  VPLAIN(s->vec, k_gm_scale, (g, TB, 0, st), s->M, d_b, s->V, &s->st->beta, s->st, 0);
  HIP_TRY(hipGetLastError());
  return PSIGNN_OK;
}

// The launch sequence of Arnoldi step j (psignn_gmres_step below; the adjoint solve at the end of this file).  `limit`: device int,
// the step count at which the cycle ends whatever the residual (NULL: none).
static void gm_step_launch(psignn_gmres* s, int j, double shift, double eta, const int32_t* limit, hipStream_t st) {
  const unsigned g = (unsigned)s->nblk;
  float* w = s->V + (size_t)(j + 1) * s->ld;
  KNOB_INT(always, [] { const char* e = getenv("PSIGNN_GMRES_REORTH"); return e && strcmp(e, "always") == 0 ? 1 : 0; }());
  for (int pass = 0; pass < 2; ++pass) {
    VLAUNCH("k_gm_dots", st, s->vec, k_gm_dots, (g, TB, 0, st), s->M, s->ld, j, 0.f, s->st, s->V, w, s->part, s->ldp, pass);
    LAUNCH("k_gm_reduce", st, (k_gm_reduce<<<(unsigned)(j + 1 + (pass == 0)), TB, 0, st>>>(s->st, s->part, s->nblk, s->ldp, s->coef, s->hcol, pass, j + 1)));
    VLAUNCH("k_gm_axpy", st, s->vec, k_gm_axpy, (g, TB, 0, st), s->M, s->ld, j, s->st, s->V, w, s->coef, s->part, s->nblk, pass);
    if (pass == 0) LAUNCH("k_gm_decide", st, (k_gm_decide<<<1, TB, 0, st>>>(s->st, s->part, s->nblk, always)));
  }
  LAUNCH("k_gm_finish", st, (k_gm_finish<<<1, TB, 0, st>>>(s->st, s->part, s->nblk, j, s->m, s->H, s->cs, s->sn, s->g, s->hcol, s->res_hist, eta, shift, limit)));
  VLAUNCH("k_gm_scale", st, s->vec, k_gm_scale, (g, TB, 0, st), s->M, w, w, &s->st->hn, s->st, 1);
}

// Arnoldi step j: basis slot j + 1 holds the caller's raw product P = (operator applied to v_j); the Krylov operator is
// A v = P - shift * v (shift = 1 for A = J_f - I).  h_done (may be NULL): synchronous read of the stop flag.
extern "C" int psignn_gmres_step(psignn_gmres_t* s, int j, double shift, double eta, int* h_done, void* stream) {
  ARG_CHECK(s && j >= 0 && j < s->m, "step index outside the basis");
  hipStream_t st = (hipStream_t)stream;
  gm_step_launch(s, j, shift, eta, nullptr, st);
  if (h_done) {
    HIP_TRY(hipMemcpyAsync(s->h_st, s->st, sizeof(GmresState), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *h_done = s->h_st->done;
  }
  HIP_TRY(hipGetLastError());
  return PSIGNN_OK;
}

// d_dst = d_base + scale * V y (y from the first k columns; k <= 0: all completed steps).  h_info: [k, beta, resid] (may be NULL)
extern "C" int psignn_gmres_solution(psignn_gmres_t* s, int k, const float* d_base, double scale, float* d_dst, double* h_info,
                                     void* stream) {
  ARG_CHECK(s && d_dst, "NULL argument");
  hipStream_t st = (hipStream_t)stream;
  k_gm_backsolve<<<1, 64, 0, st>>>(s->st, k, s->m, s->H, s->g, s->y, s->coef);
  VLAUNCH("k_gm_combine", st, s->vec, k_gm_combine, ((unsigned)s->nblk, TB, 0, st), s->M, s->ld, s->st, k, s->V, s->coef, d_base, (float)scale, d_dst);
  if (h_info) {
    HIP_TRY(hipMemcpyAsync(s->h_st, s->st, sizeof(GmresState), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    h_info[0] = (double)s->h_st->k;
    h_info[1] = s->h_st->beta;
    h_info[2] = s->h_st->resid;
  }
  HIP_TRY(hipGetLastError());
  return PSIGNN_OK;
}

// number of Arnoldi steps of the current solve whose second Gram-Schmidt pass ran (synchronous read)
extern "C" int psignn_gmres_reorth_count(psignn_gmres_t* s, int* h_count, void* stream) {
  ARG_CHECK(s && h_count, "NULL argument");
  HIP_TRY(hipMemcpyAsync(s->h_st, s->st, sizeof(GmresState), hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  *h_count = s->h_st->n_reorth;
  return PSIGNN_OK;
}

// residual history of the last solve: h_res[0] = beta, h_res[i] = |residual| after i steps (m + 1 doubles)
extern "C" int psignn_gmres_history(psignn_gmres_t* s, double* h_res, void* stream) {
  ARG_CHECK(s && h_res, "NULL argument");
  HIP_TRY(hipMemcpyAsync(h_res, s->res_hist, (size_t)(s->m + 1) * 8, hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  return PSIGNN_OK;
}

// ------------------------------------------------------------------------------------------
// Restarted GMRES for the adjoint system of the implicit backward,  y = J_f(h*)^T y + grad  <=>  (J^T - I) y = -grad
// (the reference's backward hook, dirichlet/psignn/model.py:210-223, solves this LINEAR system with Broyden).  Opt-in.
// Per restart cycle, all on the stream:
//   begin  (k_ag_begin) : f(y) = J^T y + grad, r = f(y) - y -> basis row 0, block partials of |r|^2 and |f(y)|^2.  The first cycle
//                         has y = 0: r = grad, no product.
//   check  (k_ag_check) : one block.  rel = |r| / (|f(y)| + 1e-9), the measure of the Broyden solver; traces; the solve ends on
//                         rel < eps, on rel > 1/2 of the previous cycle's rel (stagnation at the working precision) or on a spent
//                         budget.  Otherwise the Arnoldi state is re-armed: g_0 = |r|, inner target |residual| <= eps / 2 |f(y)|.
//   keep   (k_ag_keep)  : y_best = y when this cycle's rel is the lowest so far (the result is y_best).
//   Arnoldi             : up to m steps of gm_step_launch on the raw products J^T v_j (shift 1); the product runs ungated, every
//                         other kernel returns once GmresState::done is up (cycle over, or solve over).
//   end                 : y -= V z, z the least-squares solution of (J^T - I) z = r (k_gm_backsolve, k_gm_combine).
// The host reads the solve state after every check and the cycle flag every poll_every products; it only ever skips launches that
// would return at once, so the bits and the counts do not depend on poll_every.  Reductions have a fixed shape: reproducible.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ void ag_init_body(AdjState* as) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    as->cycles = 0; as->products = 0; as->done = 0; as->stop = 0; as->steps_left = 0; as->improved = 0; as->n_reorth = 0; as->pad = 0;
    as->prev_rel = 0.0; as->lowest = 0.0; as->lowest_abs = 0.0; as->rnorm = 0.0;
  }
}
__global__ void k_ag_init(AdjState* as) { ag_init_body(as); }

// r = f(y) - y -> r0, f(y) = jty + grad (first: y := 0, f(y) = grad); partials of |r|^2 and |f(y)|^2, one pair per block
template <int VEC>
__device__ __forceinline__ void ag_begin_body(int64_t M, const AdjState* __restrict__ as, float* __restrict__ y,
                                              const float* __restrict__ jty, const float* __restrict__ grad,
                                              float* __restrict__ r0, float* __restrict__ part, int nblk, int first) {
  if (as->done) return;
  int64_t e0 = elem0<VEC>();
  float sr = 0.f, sf = 0.f;
  if (e0 < M) {
    float f[VEC], a[VEC];
    ldv<VEC>(grad, e0, M, f);
    if (first) {
#pragma unroll
      for (int i = 0; i < VEC; ++i) a[i] = 0.f;
      stv<VEC>(y, e0, M, a);
    } else {
      float t[VEC];
      ldv<VEC>(jty, e0, M, t);
      ldv<VEC>(y, e0, M, a);
#pragma unroll
      for (int i = 0; i < VEC; ++i) f[i] += t[i];
    }
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      sf = fmaf(f[i], f[i], sf);
      f[i] -= a[i];
      sr = fmaf(f[i], f[i], sr);
    }
    stv<VEC>(r0, e0, M, f);
  }
  block_pair_store(sr, sf, part, nblk);
}
template <int VEC>
__global__ __launch_bounds__(TB) void k_ag_begin(int64_t M, const AdjState* __restrict__ as, float* __restrict__ y,
                                                 const float* __restrict__ jty, const float* __restrict__ grad,
                                                 float* __restrict__ r0, float* __restrict__ part, int nblk, int first) {
  ag_begin_body<VEC>(M, as, y, jty, grad, r0, part, nblk, first);
}

// One block: the stop tests of the solve and the re-arming of the cycle
// AUG, a solve with kept corrections or another stall ratio (k_lg_check): the ratio is `stall`, the last cycle's augmentation steps
// are counted and the cycle's plan is written.  The solve without options (AUG false) compiles to what it always was.
template <bool AUG>
__device__ __forceinline__ void ag_check_body(AdjState* as, GmresState* st, const float* __restrict__ part, int nblk,
                                              double* __restrict__ g, double* __restrict__ rel_trace,
                                              double* __restrict__ abs_trace, int cap, double eps, int max_products, int m,
                                              double stall, int augment) {
  __shared__ double sh[TB];
  if (as->done) return;
  const double sr = block_sum_partials(part, nblk, sh);
  const double sf = block_sum_partials(part + nblk, nblk, sh);
  if (threadIdx.x != 0) return;
  const double nr = (double)(float)sqrt(sr), nf = (double)(float)sqrt(sf);
  const double rel = nr / (nf + 1e-9);
  const int c = as->cycles;
  const int products = as->products + (c > 0 ? st->k + 1 : 0);   // the last cycle's steps and this cycle's residual
  as->products = products;
  as->cycles = c + 1;
  as->n_reorth = st->n_reorth;
  if (c < cap) {
    rel_trace[c] = rel;
    abs_trace[c] = nr;
  }
  const int better = c == 0 || rel < as->lowest;
  as->improved = better;
  if (better) {
    as->lowest = rel;
    as->lowest_abs = nr;
  }
  const int left = min(m, max_products - products - 1);
  int done = 1, stop = 0;
  if (rel < eps || nr == 0.0) stop = 1;   // (a zero right-hand side: y = 0 is the answer)
  else if (c > 0 && !(rel <= (AUG ? stall : 0.5) * as->prev_rel)) stop = 2;   // (a NaN stops here too)
  else if (left <= 0) stop = 0;
  else done = 0;
  as->prev_rel = rel;
  as->done = done;
  as->stop = stop;
  as->steps_left = done ? 0 : left;
  as->rnorm = nr;
  st->done = done;
  if (AUG && c > 0 && st->k > as->nk) as->n_aug += st->k - as->nk;
  if (AUG && !done) {
    const int ka = lgm_plan_ka(as->stored, augment, left);
    as->ka = ka;
    as->nk = left - ka;
  }
  if (!done) {
    st->k = 0; st->breakdown = 0; st->reorth = 1;
    st->beta = nf;          // k_gm_finish stops the cycle at |residual| <= eta * beta with eta = eps / 2
    st->resid = nr; st->hn = 0.0; st->n0sq = 0.0;
    g[0] = nr;
  }
}
__global__ __launch_bounds__(TB) void k_ag_check(AdjState* as, GmresState* st, const float* __restrict__ part, int nblk,
                                                 double* __restrict__ g, double* __restrict__ rel_trace,
                                                 double* __restrict__ abs_trace, int cap, double eps, int max_products, int m) {
  ag_check_body<false>(as, st, part, nblk, g, rel_trace, abs_trace, cap, eps, max_products, m, 0.5, 0);
}
__global__ __launch_bounds__(TB) void k_lg_check(AdjState* as, GmresState* st, const float* __restrict__ part, int nblk,
                                                 double* __restrict__ g, double* __restrict__ rel_trace,
                                                 double* __restrict__ abs_trace, int cap, double eps, int max_products, int m,
                                                 double stall, int augment) {
  ag_check_body<true>(as, st, part, nblk, g, rel_trace, abs_trace, cap, eps, max_products, m, stall, augment);
}

template <int VEC>
__device__ __forceinline__ void ag_keep_body(int64_t M, const AdjState* __restrict__ as, const float* __restrict__ y,
                                             float* __restrict__ ybest) {
  if (!as->improved) return;
  int64_t e0 = elem0<VEC>();
  if (e0 >= M) return;
  float x[VEC];
  ldv<VEC>(y, e0, M, x);
  stv<VEC>(ybest, e0, M, x);
}
template <int VEC>
__global__ __launch_bounds__(TB) void k_ag_keep(int64_t M, const AdjState* __restrict__ as, const float* __restrict__ y,
                                                float* __restrict__ ybest) {
  ag_keep_body<VEC>(M, as, y, ybest);
}

// ------------------------------------------------------------------------------------------
// Augmented restarts (LGMRES; Baker, Jessup, Manteuffel 2005) and the stall ratio of the restarted adjoint solve, opt-in through
// psignn_gmres_solve_adjoint_opts / _lin_opts.  The method is the one stated in the header of krylov_f64.hip, with fp32 vectors;
// tests/lgmres_ref.py restates it.  In short:
//   ring     : (the handle's augment) + 1 rows of ld floats beside the basis, caller-owned; cleared at the start of every solve
//              (k_lg_init: stored = 0).  At the end of a cycle dy = sum_j z_j s_j, y -= dy; dy / |dy| becomes the newest entry when
//              |dy| is positive and finite.  The slot that is due is never a source of the cycle that writes it.
//   plan     : k_lg_check writes ka = min(stored, augment, left - 1) and nk = left - ka (gmres_dense.h: lgm_plan_*) into AdjState.
//   aug step : j >= nk.  The product J^T zhat goes into basis row j + 1, k_lg_shift forms w -= zhat (zhat is no basis vector: the
//              shift cannot sit on the Hessenberg's diagonal), then gm_step_launch with shift 0.
//   end      : k_lg_combine reads min(k, nk) basis rows and k - min(k, nk) ring rows, writes y, the raw dy into the slot that is due
//              and the block partials of |dy|^2; k_lg_norm (one block) turns them into |dy|, the stored flag and the new head;
//              k_gm_scale divides the slot by |dy| once the next check has re-armed the flag it is gated by.
//   stop     : at the head of cycle c > 0 the solve ends when !(rel <= stall * prev_rel).
// No atomics, every scalar on the device; the host reads AdjState after a check, as it always has.  {augment 0, stall 0.5} launches
// exactly the kernels of the solve without options.
// ------------------------------------------------------------------------------------------
__global__ void k_lg_init(AdjState* as) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    as->nk = 0; as->ka = 0; as->stored = 0; as->head = 0; as->n_aug = 0; as->dy_ok = 0; as->dyn = 0.0;
  }
}

// w -= zhat in place, the head of an augmentation step: two reads, one write
template <int VEC>
__global__ __launch_bounds__(TB) void k_lg_shift(int64_t M, const GmresState* __restrict__ st, const float* __restrict__ zhat,
                                                 float* __restrict__ w) {
  if (st->done) return;
  int64_t e0 = elem0<VEC>();
  if (e0 >= M) return;
  float x[VEC], z[VEC];
  ldv<VEC>(w, e0, M, x);
  ldv<VEC>(zhat, e0, M, z);
#pragma unroll
  for (int i = 0; i < VEC; ++i) x[i] -= z[i];
  stv<VEC>(w, e0, M, x);
}

// The end of an augmented cycle (not gated: the cycle's flag is up): dy = sum_{i < min(k, nk)} coef_i v_i + sum_{nk <= i < k} coef_i
// zhat_(i - nk), the basis rows first, each list in ascending order; y -= dy; dy -> the ring slot that is due; block partials of
// |dy|^2 in part[0 .. nblk).  Z is read and written in distinct rows: the ring has one slot more than a cycle reads.
template <int VEC>
__global__ __launch_bounds__(TB) void k_lg_combine(int64_t M, int64_t ld, const GmresState* __restrict__ st,
                                                   const AdjState* __restrict__ as, const float* __restrict__ V, float* Z, int nslots,
                                                   const float* __restrict__ coef, float* __restrict__ y, float* __restrict__ part,
                                                   int nblk) {
  int64_t e0 = elem0<VEC>();
  const int k = st->k, nk = as->nk, head = as->head;
  const int kb = min(k, nk);
  float s = 0.f, zero = 0.f;
  if (e0 < M) {
    float acc[VEC];
#pragma unroll
    for (int q = 0; q < VEC; ++q) acc[q] = 0.f;
    for (int i = 0; i < kb; ++i) {
      const float c = coef[i];
      float v[VEC];
      ldv<VEC>(V + (int64_t)i * ld, e0, M, v);
#pragma unroll
      for (int q = 0; q < VEC; ++q) acc[q] = fmaf(c, v[q], acc[q]);
    }
    for (int i = nk; i < k; ++i) {
      const float c = coef[i];
      float v[VEC];
      ldv<VEC>(Z + (int64_t)lgm_slot_newest(head, nslots, i - nk) * ld, e0, M, v);
#pragma unroll
      for (int q = 0; q < VEC; ++q) acc[q] = fmaf(c, v[q], acc[q]);
    }
    float b[VEC];
    ldv<VEC>(y, e0, M, b);
#pragma unroll
    for (int q = 0; q < VEC; ++q) {
      b[q] -= acc[q];
      s = fmaf(acc[q], acc[q], s);
    }
    stv<VEC>(y, e0, M, b);
    stv<VEC>(Z + (int64_t)lgm_slot_due(head) * ld, e0, M, acc);
  }
  block_pair_store(s, zero, part, nblk);
}

// One block: n = |dy|; when n > 0 and finite the slot that was due becomes the newest entry (it holds dy until the next head of a
// cycle divides it by n) and the `augment` newest are kept.
__global__ __launch_bounds__(TB) void k_lg_norm(AdjState* as, const float* __restrict__ part, int nblk, int nslots, int augment) {
  __shared__ double sh[TB];
  const double s2 = block_sum_partials(part, nblk, sh);
  if (threadIdx.x != 0) return;
  const double n = (double)(float)sqrt(s2);
  const int ok = n > 0.0 && n < (double)INFINITY;   // (a NaN is neither)
  as->dyn = n;
  as->dy_ok = ok;
  if (ok) {
    as->head = lgm_push(as->head, nslots);
    as->stored = lgm_stored_after_push(as->stored, augment);
  }
}

using ws::AdjWork;   // work = [ operator scratch | y | J^T y | y_best | grad_p | h*_p | prb_p | normals_p | layer states ]
static AdjWork adj_work(const psignn_plan* p, int nl, float* base) { return ws::adj_work(p->N, nl, p->mixed, base); }

extern "C" int64_t psignn_gmres_adjoint_workspace_floats(const psignn_plan_t* p, int n_layers) {
  if (!p || n_layers < 1 || n_layers > 64) return -1;
  return adj_work(p, n_layers, nullptr).total;
}

static int adj_prepare(psignn_gmres* s, int max_products) {
  const int cap = max_products / 2 + 3;   // a cycle after the first spends at least two products
  if (!s->ast) {
    if (hipMalloc((void**)&s->ast, sizeof(AdjState)) != hipSuccess || hipHostMalloc((void**)&s->h_ast, sizeof(AdjState)) != hipSuccess) {
      psignn_set_error("gmres adjoint: allocation of the solve state failed");
      return PSIGNN_ENOMEM;
    }
    s->bytes += sizeof(AdjState);
  }
  if (s->a_cap < cap) {
    if (s->a_rel) (void)hipFree(s->a_rel);
    if (s->a_abs) (void)hipFree(s->a_abs);
    s->a_rel = s->a_abs = nullptr;
    s->bytes -= (size_t)s->a_cap * 16;
    s->a_cap = 0;
    if (hipMalloc((void**)&s->a_rel, (size_t)cap * 8) != hipSuccess || hipMalloc((void**)&s->a_abs, (size_t)cap * 8) != hipSuccess) {
      psignn_set_error("gmres adjoint: allocation of the traces failed");
      return PSIGNN_ENOMEM;
    }
    s->a_cap = cap;
    s->bytes += (size_t)cap * 16;
  }
  return PSIGNN_OK;
}

// The read-out at the end of a solve, single or lockstep (s->h_ast holds the final solve state): the best iterate in the caller's
// numbering (res_plan: the plan whose order the solve ran in, or NULL), the traces up to min(cycles, a_cap) entries, the counts.
static int adjoint_gmres_read_out(psignn_gmres* s, const psignn_plan* res_plan, const float* ybest, float* d_result,
                                  psignn_gmres_adjoint_info_t* info, double* h_rel, double* h_abs, hipStream_t st) {
  int rc;
  if (d_result) {
    if (res_plan) {
      if ((rc = psignn_plan_permute(res_plan, ybest, D, d_result, 0, st))) return rc;
    } else {
      HIP_TRY(hipMemcpyAsync(d_result, ybest, (size_t)s->M * 4, hipMemcpyDeviceToDevice, st));
    }
  }
  const AdjState& h = *s->h_ast;
  const int n = std::min(h.cycles, s->a_cap);
  if (h_rel && n > 0) HIP_TRY(hipMemcpyAsync(h_rel, s->a_rel, (size_t)n * 8, hipMemcpyDeviceToHost, st));
  if (h_abs && n > 0) HIP_TRY(hipMemcpyAsync(h_abs, s->a_abs, (size_t)n * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (info) {
    info->products = h.products;
    info->cycles = h.cycles;
    info->stop_reason = h.stop;
    info->n_reorth = h.n_reorth;
    info->lowest = h.lowest;
    info->lowest_abs = h.lowest_abs;
  }
  HIP_TRY(hipGetLastError());
  return PSIGNN_OK;
}

// vjp(w, out): out = J_f(h*)^T w in the solve's numbering.  grad, y, fy, ybest: that numbering too.  res_plan: the plan whose order the
// solve runs in (the result goes back to the caller's numbering), or NULL.
// o: {0, 0.5} is the solve without options; anything else keeps corrections in the handle's ring and / or tests the stall ratio
// (the k_lg_* kernels above).  h_n_aug (may be NULL): the augmentation steps of the solve.
static const psignn_gmres_opts_t GM_PLAIN = {0, 0.5};
static int adjoint_opts_check(const char* who, const psignn_gmres* s, const psignn_gmres_opts_t* o) {
  ARG_CHECK_AS(who, s && o, "NULL argument");
  ARG_CHECK_AS(who, o->augment >= 0 && o->augment <= s->augment, "augment out of range (0 .. the handle's augment)");
  ARG_CHECK_AS(who, o->stall > 0.0 && o->stall <= 1.0, "stall must be in (0, 1]");   // (a NaN is not)
  return PSIGNN_OK;
}
template <class F>
static int adjoint_gmres_loop(psignn_gmres* s, const float* grad, double eps, int max_products, int poll_every, F&& vjp, const AdjWork& w,
                              const psignn_plan* res_plan, float* d_result, psignn_gmres_adjoint_info_t* info, double* h_rel,
                              double* h_abs, hipStream_t st, const psignn_gmres_opts_t& o = GM_PLAIN, int32_t* h_n_aug = nullptr) {
  if (poll_every <= 0) poll_every = 8;
  int rc = adj_prepare(s, max_products);
  if (rc) return rc;
  const unsigned g = (unsigned)s->nblk;
  const int64_t vb = s->M * 4;
  const int aug = o.augment, nslots = s->augment + 1;
  const bool plain = aug == 0 && o.stall == 0.5;   // the launches of the solve without options
  k_gm_init<<<4, TB, 0, st>>>(s->st, s->g, s->res_hist, s->m);
  k_ag_init<<<1, 64, 0, st>>>(s->ast);
  if (!plain) k_lg_init<<<1, 64, 0, st>>>(s->ast);
  for (int cycle = 0;; ++cycle) {
    if (cycle > 0 && (rc = vjp(w.y, w.fy))) return rc;
    PROF_BYTES(cycle ? 4 * vb : 3 * vb);
    VLAUNCH("k_ag_begin", st, s->vec, k_ag_begin, (g, TB, 0, st), s->M, s->ast, w.y, w.fy, grad, s->V, s->part, s->nblk, cycle == 0);
    if (plain)
      LAUNCH("k_ag_check", st, (k_ag_check<<<1, TB, 0, st>>>(s->ast, s->st, s->part, s->nblk, s->g, s->a_rel, s->a_abs, s->a_cap, eps,
                                                            max_products, s->m)));
    else
      LAUNCH("k_lg_check", st, (k_lg_check<<<1, TB, 0, st>>>(s->ast, s->st, s->part, s->nblk, s->g, s->a_rel, s->a_abs, s->a_cap, eps,
                                                            max_products, s->m, o.stall, aug)));
    PROF_BYTES(2 * vb);
    VLAUNCH("k_ag_keep", st, s->vec, k_ag_keep, (g, TB, 0, st), s->M, s->ast, w.y, w.ybest);
    VLAUNCH("k_gm_scale", st, s->vec, k_gm_scale, (g, TB, 0, st), s->M, s->V, s->V, &s->ast->rnorm, s->st, 1);
    HIP_TRY(hipMemcpyAsync(s->h_ast, s->ast, sizeof(AdjState), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (s->h_ast->done) break;
    const int steps = s->h_ast->steps_left;
    // the cycle's plan and the ring as the check left them (no kept corrections: all Krylov steps)
    const int nk = aug ? s->h_ast->nk : steps, head = aug ? s->h_ast->head : 0;
    if (steps < 1 || steps > s->m || nk < 1 || nk > steps || steps - nk > aug || head < 0 || head >= nslots) {
      psignn_set_error("gmres adjoint: internal: plan of %d Krylov steps out of %d (restart length %d), %d kept, ring head %d of %d", nk,
                       steps, s->m, aug, head, nslots);
      return PSIGNN_EHIP;
    }
    if (aug && cycle > 0 && s->h_ast->dy_ok) {   // zhat = dy / |dy|: the newest slot still holds the last cycle's dy
      float* zn = s->Z + (size_t)lgm_slot_newest(head, nslots, 0) * s->ld;
      PROF_BYTES(2 * vb);
      VLAUNCH("k_gm_scale", st, s->vec, k_gm_scale, (g, TB, 0, st), s->M, zn, zn, &s->ast->dyn, s->st, 1);
    }
    for (int j = 0; j < steps; ++j) {
      float* wj = s->V + (size_t)(j + 1) * s->ld;
      const float* src = j < nk ? s->V + (size_t)j * s->ld : s->Z + (size_t)lgm_slot_newest(head, nslots, j - nk) * s->ld;
      if ((rc = vjp(src, wj))) return rc;
      if (j >= nk) {
        PROF_BYTES(3 * vb);
        VLAUNCH("k_lg_shift", st, s->vec, k_lg_shift, (g, TB, 0, st), s->M, s->st, src, wj);
      }
      gm_step_launch(s, j, j < nk ? 1.0 : 0.0, 0.5 * eps, &s->ast->steps_left, st);
      if ((j + 1) % poll_every == 0 && j + 1 < steps) {
        HIP_TRY(hipMemcpyAsync(s->h_st, s->st, sizeof(GmresState), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (s->h_st->done) break;
      }
    }
    LAUNCH("k_gm_backsolve", st, (k_gm_backsolve<<<1, 64, 0, st>>>(s->st, 0, s->m, s->H, s->g, s->y, s->coef)));
    if (!aug) {
      VLAUNCH("k_gm_combine", st, s->vec, k_gm_combine, (g, TB, 0, st), s->M, s->ld, s->st, 0, s->V, s->coef, w.y, -1.f, w.y);
    } else {
      PROF_BYTES(((int64_t)steps + 3) * vb);
      VLAUNCH("k_lg_combine", st, s->vec, k_lg_combine, (g, TB, 0, st), s->M, s->ld, s->st, s->ast, s->V, s->Z, nslots, s->coef, w.y,
              s->part, s->nblk);
      LAUNCH("k_lg_norm", st, (k_lg_norm<<<1, TB, 0, st>>>(s->ast, s->part, s->nblk, nslots, aug)));
    }
  }
  if (h_n_aug) *h_n_aug = plain ? 0 : s->h_ast->n_aug;
  return adjoint_gmres_read_out(s, res_plan, w.ybest, d_result, info, h_rel, h_abs, st);
}

static int adjoint_direct(const char* who, psignn_gmres_t* s, const psignn_plan_t* p, const float* W, int nl, const float* h_star,
                          const float* prb, const float* nrm, const float* grad, double eps, int max_products, int poll_every,
                          const psignn_gmres_opts_t& o, float* d_work, float* d_result, psignn_gmres_adjoint_info_t* info,
                          int32_t* h_n_aug, double* h_rel, double* h_abs, void* stream) {
  ARG_CHECK_AS(who, s && p && W && h_star && prb && grad && d_work, "NULL argument");
  ARG_CHECK_AS(who, s->M == p->N * D, "the GMRES handle was made for another vector length than the plan's N * d");
  ARG_CHECK_AS(who, nl >= 1 && nl <= 64, "n_layers out of range");
  ARG_CHECK_AS(who, !p->mixed || nrm, "mixed plan needs unit normals");
  ARG_CHECK_AS(who, max_products >= 1 && eps >= 0.0, "max_products >= 1, eps >= 0");
  hipStream_t st = (hipStream_t)stream;
  const AdjWork w = adj_work(p, nl, d_work);
  AdjointOp op;   // tiled plans: the whole solve in plan order; otherwise the caller's numbering
  int rc = op.setup(p, W, nl, h_star, prb, nrm, grad, ws::Adapter{w.fwork, w.hs_p, w.grad_p, nullptr, w.prbp, w.nrmp}, w.fwork, w.lwork, st);
  if (rc) return rc;
  return adjoint_gmres_loop(s, op.grad, eps, max_products, poll_every, op, w, op.tiled ? p : nullptr, d_result, info, h_rel, h_abs, st, o,
                            h_n_aug);
}
extern "C" int psignn_gmres_solve_adjoint(psignn_gmres_t* s, const psignn_plan_t* p, const float* W, int nl, const float* h_star,
                                          const float* prb, const float* nrm, const float* grad, double eps, int max_products,
                                          int poll_every, float* d_work, float* d_result, psignn_gmres_adjoint_info_t* info,
                                          double* h_rel, double* h_abs, void* stream) {
  return adjoint_direct(__func__, s, p, W, nl, h_star, prb, nrm, grad, eps, max_products, poll_every, GM_PLAIN, d_work, d_result, info,
                        nullptr, h_rel, h_abs, stream);
}
// The read-out of a solve with options: psignn_gmres_adjoint_info_t's fields plus n_aug
static void gm_opts_info(const psignn_gmres_adjoint_info_t& i, int32_t n_aug, psignn_gmres_info_t* o) {
  o->products = i.products;
  o->cycles = i.cycles;
  o->stop_reason = i.stop_reason;
  o->n_reorth = i.n_reorth;
  o->lowest = i.lowest;
  o->lowest_abs = i.lowest_abs;
  o->n_aug = n_aug;
}
extern "C" int psignn_gmres_solve_adjoint_opts(psignn_gmres_t* s, const psignn_plan_t* p, const float* W, int nl, const float* h_star,
                                               const float* prb, const float* nrm, const float* grad, double eps, int max_products,
                                               int poll_every, const psignn_gmres_opts_t* opts, float* d_work, float* d_result,
                                               psignn_gmres_info_t* info, double* h_rel, double* h_abs, void* stream) {
  int rc = adjoint_opts_check(__func__, s, opts);   // (before any launch)
  if (rc) return rc;
  psignn_gmres_adjoint_info_t i{};
  int32_t n_aug = 0;
  rc = adjoint_direct(__func__, s, p, W, nl, h_star, prb, nrm, grad, eps, max_products, poll_every, *opts, d_work, d_result, &i, &n_aug,
                      h_rel, h_abs, stream);
  if (rc == PSIGNN_OK && info) gm_opts_info(i, n_aug, info);
  return rc;
}

static int adjoint_lin(const char* who, psignn_gmres_t* s, const psignn_lin_t* lin, const float* W, int nl, const float* grad, double eps,
                       int max_products, int poll_every, const psignn_gmres_opts_t& o, float* d_work, float* d_result,
                       psignn_gmres_adjoint_info_t* info, int32_t* h_n_aug, double* h_rel, double* h_abs, void* stream) {
  ARG_CHECK_AS(who, s && lin && W && grad && d_work, "NULL argument");
  const psignn_plan* p = psignn_lin_plan(lin);
  ARG_CHECK_AS(who, p && s->M == p->N * D, "the GMRES handle was made for another vector length than the linearisation's plan");
  ARG_CHECK_AS(who, nl >= 1 && nl <= 64, "n_layers out of range");
  ARG_CHECK_AS(who, max_products >= 1 && eps >= 0.0, "max_products >= 1, eps >= 0");
  hipStream_t st = (hipStream_t)stream;
  const AdjWork w = adj_work(p, nl, d_work);
  int rc;
  if ((rc = psignn_plan_permute(p, grad, D, w.grad_p, 1, st))) return rc;
  auto vjp = [&](const float* y, float* out) { return psignn_lin_vjp(lin, W, nl, y, out, w.fwork, st); };
  return adjoint_gmres_loop(s, w.grad_p, eps, max_products, poll_every, vjp, w, p, d_result, info, h_rel, h_abs, st, o, h_n_aug);
}
extern "C" int psignn_gmres_solve_adjoint_lin(psignn_gmres_t* s, const psignn_lin_t* lin, const float* W, int nl, const float* grad,
                                              double eps, int max_products, int poll_every, float* d_work, float* d_result,
                                              psignn_gmres_adjoint_info_t* info, double* h_rel, double* h_abs, void* stream) {
  return adjoint_lin(__func__, s, lin, W, nl, grad, eps, max_products, poll_every, GM_PLAIN, d_work, d_result, info, nullptr, h_rel, h_abs,
                     stream);
}
extern "C" int psignn_gmres_solve_adjoint_lin_opts(psignn_gmres_t* s, const psignn_lin_t* lin, const float* W, int nl, const float* grad,
                                                   double eps, int max_products, int poll_every, const psignn_gmres_opts_t* opts,
                                                   float* d_work, float* d_result, psignn_gmres_info_t* info, double* h_rel,
                                                   double* h_abs, void* stream) {
  int rc = adjoint_opts_check(__func__, s, opts);   // (before any launch)
  if (rc) return rc;
  psignn_gmres_adjoint_info_t i{};
  int32_t n_aug = 0;
  rc = adjoint_lin(__func__, s, lin, W, nl, grad, eps, max_products, poll_every, *opts, d_work, d_result, &i, &n_aug, h_rel, h_abs, stream);
  if (rc == PSIGNN_OK && info) gm_opts_info(i, n_aug, info);
  return rc;
}

// ------------------------------------------------------------------------------------------
// Lockstep form of the restarted adjoint solve for the replicas of one shard (the R replicas of the reference's DataParallel training
// step, */psignn/main.py:106, each running the backward hook of model.py:210-223).  The cycles are aligned across the replicas: every
// kernel above is launched ONCE per pass with blockIdx.z = replica; a block loads its replica's GmresBatchDesc (common.h) and runs the
// single-handle body on it -- same block -> element mapping, same partial-sum shapes, same reduction order --, so every replica has
// the bits of psignn_gmres_solve_adjoint_lin on the same handle.  The gates are the single kernels', per replica (AdjState::done,
// GmresState::done, reorth, improved): a replica whose solve or cycle is over costs one descriptor load per block.  The grid's x
// extent is the largest nblk of the shard; a block past its replica's extent returns.  Products: k_vjp_lin_batch on a device table
// of (m + 2) rows of n LinBatchDesc, uploaded once per solve -- row j < m maps basis row j to row j + 1 and is gated by the replica's
// GmresState, the last row maps y to J^T y and is gated by its AdjState.
// ------------------------------------------------------------------------------------------
__global__ void k_gm_init_batch(const GmresBatchDesc* __restrict__ descs) {
  const GmresBatchDesc& d = descs[blockIdx.z];
  gm_init_body(d.st, d.g, d.res_hist, d.m, blockDim.x, gridDim.x);
}
__global__ void k_ag_init_batch(const GmresBatchDesc* __restrict__ descs) { ag_init_body(descs[blockIdx.z].ast); }

template <int VEC>
__global__ __launch_bounds__(TB) void k_ag_begin_batch(const GmresBatchDesc* __restrict__ descs, int first) {
  const GmresBatchDesc& d = descs[blockIdx.z];
  if ((int)blockIdx.x >= d.nblk) return;
  ag_begin_body<VEC>(d.M, d.ast, d.yv, d.fy, d.grad, d.V, d.part, d.nblk, first);
}
// (a replica whose solve ended in an earlier cycle: `improved` is lowered, so that the keep pass of this and every later cycle
// returns at once instead of copying the unchanged iterate again)
__global__ __launch_bounds__(TB) void k_ag_check_batch(const GmresBatchDesc* __restrict__ descs, double eps, int max_products) {
  const GmresBatchDesc& d = descs[blockIdx.z];
  if (d.ast->done) {
    if (threadIdx.x == 0) d.ast->improved = 0;
    return;
  }
  ag_check_body<false>(d.ast, d.st, d.part, d.nblk, d.g, d.rel_trace, d.abs_trace, d.cap, eps, max_products, d.m, 0.5, 0);
}
template <int VEC>
__global__ __launch_bounds__(TB) void k_ag_keep_batch(const GmresBatchDesc* __restrict__ descs) {
  const GmresBatchDesc& d = descs[blockIdx.z];
  if ((int)blockIdx.x >= d.nblk) return;
  ag_keep_body<VEC>(d.M, d.ast, d.yv, d.ybest);
}
// row 0: the cycle's residual divided by AdjState::rnorm; row j + 1 of Arnoldi step j: divided by GmresState::hn
template <int VEC>
__global__ __launch_bounds__(TB) void k_gm_scale_batch(const GmresBatchDesc* __restrict__ descs, int row) {
  const GmresBatchDesc& d = descs[blockIdx.z];
  if ((int)blockIdx.x >= d.nblk) return;
  float* w = d.V + (int64_t)row * d.ld;
  gm_scale_body<VEC>(d.M, w, w, row == 0 ? &d.ast->rnorm : &d.st->hn, d.st, 1);
}
template <int VEC>
__global__ __launch_bounds__(TB) void k_gm_dots_batch(const GmresBatchDesc* __restrict__ descs, int j, int pass) {
  const GmresBatchDesc& d = descs[blockIdx.z];
  if ((int)blockIdx.x >= d.nblk) return;
  gm_dots_body<VEC>(d.M, d.ld, j, 0.f, d.st, d.V, d.V + (int64_t)(j + 1) * d.ld, d.part, d.ldp, pass);
}
__global__ __launch_bounds__(TB) void k_gm_reduce_batch(const GmresBatchDesc* __restrict__ descs, int accumulate, int n_coef) {
  const GmresBatchDesc& d = descs[blockIdx.z];
  gm_reduce_body(d.st, d.part, d.nblk, d.ldp, d.coef, d.hcol, accumulate, n_coef);
}
template <int VEC>
__global__ __launch_bounds__(TB) void k_gm_axpy_batch(const GmresBatchDesc* __restrict__ descs, int j, int pass) {
  const GmresBatchDesc& d = descs[blockIdx.z];
  if ((int)blockIdx.x >= d.nblk) return;
  gm_axpy_body<VEC>(d.M, d.ld, j, d.st, d.V, d.V + (int64_t)(j + 1) * d.ld, d.coef, d.part, d.nblk, pass);
}
__global__ __launch_bounds__(TB) void k_gm_decide_batch(const GmresBatchDesc* __restrict__ descs, int always) {
  const GmresBatchDesc& d = descs[blockIdx.z];
  gm_decide_body(d.st, d.part, d.nblk, always);
}
__global__ __launch_bounds__(TB) void k_gm_finish_batch(const GmresBatchDesc* __restrict__ descs, int j, double eta, double shift) {
  const GmresBatchDesc& d = descs[blockIdx.z];
  gm_finish_body(d.st, d.part, d.nblk, j, d.m, d.H, d.cs, d.sn, d.g, d.hcol, d.res_hist, eta, shift, &d.ast->steps_left);
}
// end of a cycle: y -= V z.  (The single solve leaves its loop before these two once the solve is over; here the replica's blocks return.)
__global__ void k_gm_backsolve_batch(const GmresBatchDesc* __restrict__ descs) {
  const GmresBatchDesc& d = descs[blockIdx.z];
  if (d.ast->done) return;
  gm_backsolve_body(d.st, 0, d.m, d.H, d.g, d.y, d.coef);
}
template <int VEC>
__global__ __launch_bounds__(TB) void k_gm_combine_batch(const GmresBatchDesc* __restrict__ descs) {
  const GmresBatchDesc& d = descs[blockIdx.z];
  if ((int)blockIdx.x >= d.nblk || d.ast->done) return;
  gm_combine_body<VEC>(d.M, d.ld, d.st, 0, d.V, d.coef, d.yv, -1.f, d.yv);
}
// after a cycle's check: out[2 r] = replica r's AdjState::done, out[2 r + 1] = its steps_left
__global__ void k_ag_gather_batch(const GmresBatchDesc* __restrict__ descs, int n, int32_t* __restrict__ out) {
  for (int r = threadIdx.x; r < n; r += blockDim.x) {
    out[2 * r] = descs[r].ast->done;
    out[2 * r + 1] = descs[r].ast->steps_left;
  }
}
// *all_done = 1 when every replica's cycle is over (kb_all_done of the batched Broyden solve, on GmresState::done)
__global__ void k_gm_all_done_batch(const GmresBatchDesc* __restrict__ descs, int n, int32_t* __restrict__ all_done) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    int a = 1;
    for (int r = 0; r < n; ++r) a &= descs[r].st->done != 0;
    *all_done = a;
  }
}

// 1 when psignn_gmres_solve_adjoint_lin_batch takes these handles and linearisations together: one vector width and one restart
// length, every lins[i] built and of a form the batched product takes (psignn_lin_batch_ok), handle i made for the length of lins[i]'s
// plan, all plans of one family.  A host-side question; 0 also for NULL arguments.
extern "C" int psignn_gmres_adjoint_batchable(int n, psignn_gmres_t* const* sv, const psignn_lin_t* const* lins) {
  if (n <= 0 || !sv || !lins) return 0;
  for (int r = 0; r < n; ++r) {
    if (!sv[r] || !lins[r]) return 0;
    const psignn_plan* p = psignn_lin_plan(lins[r]);
    if (!p || !psignn_lin_batch_ok(lins[r], p)) return 0;
    if (sv[r]->vec != sv[0]->vec || sv[r]->m != sv[0]->m) return 0;
    if (sv[r]->M != p->N * D) return 0;
    if (p->mixed != psignn_lin_plan(lins[0])->mixed) return 0;
    for (int q = 0; q < r; ++q)
      if (sv[q] == sv[r]) return 0;   // one handle per replica: its state cannot serve two
  }
  return 1;
}

// The batched launch sequence of Arnoldi step j (gm_step_launch, one launch per pass over the shard).  The step has no schedule to
// decide -- seven launches, no forms, no stated bytes --, so the two sequences stand side by side instead of behind a chain and two targets.
static void gm_step_launch_batch(const GmresBatchDesc* dd, int n, int vec, unsigned max_g, int j, double shift, double eta,
                                 hipStream_t st) {
  const dim3 gv(max_g, 1, (unsigned)n);
  KNOB_INT(always, [] { const char* e = getenv("PSIGNN_GMRES_REORTH"); return e && strcmp(e, "always") == 0 ? 1 : 0; }());
  for (int pass = 0; pass < 2; ++pass) {
    VLAUNCH("k_gm_dots_batch", st, vec, k_gm_dots_batch, (gv, TB, 0, st), dd, j, pass);
    LAUNCH("k_gm_reduce_batch", st, (k_gm_reduce_batch<<<dim3((unsigned)(j + 1 + (pass == 0)), 1, (unsigned)n), TB, 0, st>>>(dd, pass, j + 1)));
    VLAUNCH("k_gm_axpy_batch", st, vec, k_gm_axpy_batch, (gv, TB, 0, st), dd, j, pass);
    if (pass == 0) LAUNCH("k_gm_decide_batch", st, (k_gm_decide_batch<<<dim3(1, 1, (unsigned)n), TB, 0, st>>>(dd, always)));
  }
  LAUNCH("k_gm_finish_batch", st, (k_gm_finish_batch<<<dim3(1, 1, (unsigned)n), TB, 0, st>>>(dd, j, eta, shift)));
  VLAUNCH("k_gm_scale_batch", st, vec, k_gm_scale_batch, (gv, TB, 0, st), dd, j + 1);
}

extern "C" int psignn_gmres_solve_adjoint_lin_batch(int n, psignn_gmres_t** sv, const psignn_lin_t* const* lins, const float* W, int nl,
                                                    const float* const* grads, double eps, int max_products, int poll_every,
                                                    float* const* d_works, float* const* d_results,
                                                    psignn_gmres_adjoint_info_t* infos, double* const* h_rel, double* const* h_abs,
                                                    void* stream) {
  ARG_CHECK(n > 0 && sv && lins && W && grads && d_works, "bad arguments");
  ARG_CHECK(nl == 1, "the batched adjoint solve runs single-layer blocks");
  ARG_CHECK(max_products >= 1 && eps >= 0.0, "max_products >= 1, eps >= 0");
  // (nothing is launched for a shard the lockstep does not take)
  ARG_CHECK(psignn_gmres_adjoint_batchable(n, sv, lins),
            "batched GMRES adjoint solve: handles / linearisations are not batchable (psignn_gmres_adjoint_batchable)");
  for (int r = 0; r < n; ++r) ARG_CHECK(grads[r] && d_works[r], "NULL argument");
  hipStream_t st = (hipStream_t)stream;
  if (poll_every <= 0) poll_every = 8;
  const int m = sv[0]->m, vec = sv[0]->vec;
  const int mixed = psignn_lin_plan(lins[0])->mixed;
  int rc;
  for (int r = 0; r < n; ++r)
    if ((rc = adj_prepare(sv[r], max_products))) return rc;
  // ---- per replica: the lazy work of the transposed product, the permuted right-hand side, its descriptor and its column of the
  // product table
  std::vector<GmresBatchDesc> hd(n);
  std::vector<LinBatchDesc> tab((size_t)(m + 2) * n);
  std::vector<AdjWork> works(n);
  int max_rows = 0, n_slots = 0, max_g = 0;
  int64_t bv_tot = 0, vb_tot = 0;   // bytes of one transposed product / of one state vector, summed over the shard (profiling records)
  for (int r = 0; r < n; ++r) {
    psignn_gmres* s = sv[r];
    const psignn_plan* p = psignn_lin_plan(lins[r]);
    const AdjWork w = works[r] = adj_work(p, 1, d_works[r]);
    LinBatchDesc l;
    if ((rc = psignn_lin_batch_fill(lins[r], &l, st))) return rc;
    if ((rc = psignn_plan_permute(p, grads[r], D, w.grad_p, 1, st))) return rc;
    bv_tot += psignn_lin_vjp_bytes(lins[r]);
    vb_tot += s->M * 4;
    max_rows = std::max(max_rows, p->max_rows);
    max_g = std::max(max_g, s->nblk);
    GmresBatchDesc& d = hd[r];
    d.M = s->M; d.ld = s->ld; d.nblk = s->nblk; d.ldp = s->ldp; d.m = s->m; d.cap = s->a_cap;
    d.V = s->V; d.part = s->part; d.coef = s->coef;
    d.H = s->H; d.cs = s->cs; d.sn = s->sn; d.g = s->g; d.hcol = s->hcol; d.y = s->y; d.res_hist = s->res_hist;
    d.st = s->st; d.ast = s->ast;
    d.yv = w.y; d.fy = w.fy; d.ybest = w.ybest; d.grad = w.grad_p;
    d.rel_trace = s->a_rel; d.abs_trace = s->a_abs;
    l.slot_base = n_slots;
    n_slots += l.n_slots;
    for (int j = 0; j < m; ++j) {   // Arnoldi step j: basis row j -> row j + 1, skipped once the replica's cycle is over
      LinBatchDesc& t = tab[(size_t)j * n + r];
      t = l;
      t.w = s->V + (size_t)j * s->ld;
      t.out = s->V + (size_t)(j + 1) * s->ld;
      t.st = reinterpret_cast<const int32_t*>(s->st);
    }
    for (int j = m; j < m + 2; ++j) {   // the last row: the cycle's residual product y -> J^T y, skipped once the replica's solve is over
      LinBatchDesc& t = tab[(size_t)j * n + r];
      t = l;
      t.w = w.y;
      t.out = w.fy;
      t.st = reinterpret_cast<const int32_t*>(s->ast);
    }
  }
  const int off_cycle = offsetof(GmresState, done) / 4, off_solve = offsetof(AdjState, done) / 4;
  DeviceArray<GmresBatchDesc> descs_mem;
  DeviceArray<LinBatchDesc> tab_mem;
  DeviceArray<int32_t> d_flags_mem;   // [2 r] done, [2 r + 1] steps_left; [2 n] every cycle over
  PinnedArray<int32_t> h_flags_mem;
  HIP_TRY(descs_mem.alloc(n));
  HIP_TRY(tab_mem.alloc(tab.size()));
  HIP_TRY(d_flags_mem.alloc(2 * n + 1));
  HIP_TRY(h_flags_mem.alloc(2 * n + 1));
  GmresBatchDesc* const d_descs = descs_mem.get();
  LinBatchDesc* const d_tab = tab_mem.get();
  int32_t *const d_flags = d_flags_mem.get(), *const h_flags = h_flags_mem.get();
  if ((rc = upload_wait(d_descs, hd.data(), hd.size(), st))) return rc;
  if ((rc = upload_wait(d_tab, tab.data(), tab.size(), st))) return rc;
  const dim3 gv((unsigned)max_g, 1, (unsigned)n), g1(1, 1, (unsigned)n);
  k_gm_init_batch<<<dim3(4, 1, (unsigned)n), TB, 0, st>>>(d_descs);
  k_ag_init_batch<<<g1, 64, 0, st>>>(d_descs);
  for (int cycle = 0;; ++cycle) {
    if (cycle > 0) {
      PROF_BYTES(bv_tot);
      rc = psignn_lin_vjp_batch(d_tab + (size_t)(m + 1) * n, n, n_slots, max_rows, W, mixed, off_solve, st);
      if (rc) return rc;
    }
    PROF_BYTES(cycle ? 4 * vb_tot : 3 * vb_tot);
    VLAUNCH("k_ag_begin_batch", st, vec, k_ag_begin_batch, (gv, TB, 0, st), d_descs, cycle == 0);
    LAUNCH("k_ag_check_batch", st, (k_ag_check_batch<<<g1, TB, 0, st>>>(d_descs, eps, max_products)));
    PROF_BYTES(2 * vb_tot);
    VLAUNCH("k_ag_keep_batch", st, vec, k_ag_keep_batch, (gv, TB, 0, st), d_descs);
    VLAUNCH("k_gm_scale_batch", st, vec, k_gm_scale_batch, (gv, TB, 0, st), d_descs, 0);
    k_ag_gather_batch<<<1, 64, 0, st>>>(d_descs, n, d_flags);
    HIP_TRY(hipMemcpyAsync(h_flags, d_flags, (size_t)(2 * n) * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    int steps = 0;   // the largest allowance among the replicas still solving; 0: all are done
    for (int r = 0; r < n; ++r)
      if (!h_flags[2 * r]) steps = std::max(steps, h_flags[2 * r + 1]);
    if (steps <= 0) break;
    for (int j = 0; j < steps; ++j) {
      PROF_BYTES(bv_tot);
      rc = psignn_lin_vjp_batch(d_tab + (size_t)j * n, n, n_slots, max_rows, W, mixed, off_cycle, st);
      if (rc) return rc;
      gm_step_launch_batch(d_descs, n, vec, (unsigned)max_g, j, 1.0, 0.5 * eps, st);
      if ((j + 1) % poll_every == 0 && j + 1 < steps) {
        k_gm_all_done_batch<<<1, 64, 0, st>>>(d_descs, n, d_flags + 2 * n);
        HIP_TRY(hipMemcpyAsync(h_flags + 2 * n, d_flags + 2 * n, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (h_flags[2 * n]) break;
      }
    }
    LAUNCH("k_gm_backsolve_batch", st, (k_gm_backsolve_batch<<<g1, 64, 0, st>>>(d_descs)));
    VLAUNCH("k_gm_combine_batch", st, vec, k_gm_combine_batch, (gv, TB, 0, st), d_descs);
  }
  // ---- per replica what adjoint_gmres_loop gives
  for (int r = 0; r < n; ++r) HIP_TRY(hipMemcpyAsync(sv[r]->h_ast, sv[r]->ast, sizeof(AdjState), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  for (int r = 0; r < n; ++r)
    if ((rc = adjoint_gmres_read_out(sv[r], psignn_lin_plan(lins[r]), works[r].ybest, d_results ? d_results[r] : nullptr,
                                     infos ? &infos[r] : nullptr, h_rel ? h_rel[r] : nullptr, h_abs ? h_abs[r] : nullptr, st)))
      return rc;
  return PSIGNN_OK;
}
