// Restarted GMRES in float64 for the adjoint system of the implicit backward, y = J_f(h*)^T y + grad, every scalar on the device
// (gfx950): the float64 adjoint at any size -- what AdjointProblem.truth() of tests/adjoint_gmres_ref.py is on the CPU oracle.
//
// replaces: the backward hook's solve run in double precision (dirichlet/psignn/model.py:210-223; the reference solves this LINEAR
//           system with Broyden, psignn_broyden64_solve_adjoint is that).  The cycle logic is gmres_adjoint of
//           tests/adjoint_gmres_ref.py statement by statement, which is also what adjoint_gmres_loop of krylov.hip does in fp32.
//
// Per restart cycle, all on the stream (the map is psignn_f64_vjp with add = grad, fgnn_f64_deriv.hip):
//   k_ag64_begin   f(y) = J^T y + grad (first cycle: y = 0, f = grad, no product), r = f(y) - y -> basis row 0, block partials of
//                  |r|^2 and |f(y)|^2
//   k_ag64_check   one block: rel = |r| / (|f(y)| + 1e-9), traces, lowest; the solve ends on rel < eps (or r = 0), on a cycle that
//                  did not halve rel, or on a spent budget (one product is kept back for the next cycle's residual); otherwise the
//                  cycle is armed: g_0 = |r|, steps_left = min(m, budget left)
//   k_ag64_keep    y_best <- y when this cycle's rel is the lowest so far
//   k_gm64_scale   v_0 = r / |r|
//   Arnoldi step j on the raw product w = J^T v_j in basis row j + 1 (the shift sits on the Hessenberg's diagonal):
//     k_gm64_dots    pass 1: h_i = <v_i, w>, i <= j, and |w|^2 -- a chunk of 1024 elements of w in LDS, a wave per basis vector,
//                    16 bytes per lane, the basis read once
//     k_gm64_reduce  one block per coefficient: the chunk partials in a fixed order
//     k_gm64_axpy    w -= sum_i h_i v_i, 16 bytes per lane, the basis read once; block partials of |w'|^2
//     k_gm64_decide  one block: the second pass runs when |w'|^2 < 1/2 |w|^2 (Daniel-Gragg-Kaufman-Stewart), decided here
//     k_gm64_dots / k_gm64_reduce / k_gm64_axpy once more when it does (they return at once when it does not)
//     k_gm64_finish  one block: column j = h1 + h2 - e_j, |w|; gmres_dense.h: earlier rotations, the new one, g; the cycle ends on
//                    |g_{j+1}| <= eps / 2 |f(y)|, on steps_left or on |w| = 0
//     k_gm64_scale   v_{j+1} = w / |w|
//   k_gm64_backsolve, k_gm64_combine   z = R^{-1} g, y -= V z
// Every kernel of the Arnoldi step, the product included, returns at once when the cycle's done flag is up, so what the host has
// queued past the end of a cycle changes nothing.  The host reads the solve state after every check and the cycle flag every
// poll_every Arnoldi steps: neither bits nor counts depend on poll_every.  Reductions (f64_common.h): per-wave / per-block partials,
// then one block sums the partials, all in a fixed order: the same call gives the same bits.
// Storage: vectors, basis (m + 1, M), coefficients and partials in float64.
//
// psignn_gmres64_solve_shifted is the same loop on shift * delta = A delta + b, A = J_f(h) (psignn_f64_jvp) or J_f(h)^T, for the
// Newton step of newton_f64.hip: k_ag64_begin<true> forms r = (A delta + b) - shift * delta from the raw product and the partials of
// |r|^2 and |b|^2, k_ag64_check<true> tests the linear measure |r| / |b| <= eta, k_gm64_finish puts `shift` on the diagonal (the
// adjoint solve passes 1.0, which rounds as h - 1 always did) and ends a cycle on |g_{j+1}| <= eta |b| (the adjoint solve: eps / 2).  The Newton loop's three vector kernels live at the end of this unit.
//
// Augmented restarts (LGMRES; Baker, Jessup, Manteuffel 2005) and the stall ratio, opt-in through the *_opts entry points; both
// systems, S = shift.  tests/lgmres_ref.py restates this statement by statement.
//   Ring of corrections.  Cleared at the start of every solve (k_ag64_init: stored = 0).  At the end of a cycle that took kk >= 1
//     steps the correction is dy = sum_{j < kk} z_j s_j and y <- y - dy; n = |dy| from block partials in the fixed order of
//     f64_common.h; when n > 0 and finite, zhat = dy / n becomes the newest entry and the `augment` newest are kept.
//   Cycle plan, decided by k_lg64_check at the head of a cycle and written into G64State: `left` as ever,
//     ka = min(stored, augment, left - 1), nk = left - ka (gmres_dense.h: lgm_plan_*).  At least one Krylov step always runs.
//   Krylov step, j < nk: the step above, s_j = v_j.
//   Augmentation step, j >= nk: s_j = the (j - nk)-th newest zhat; the product A zhat goes into basis row j + 1; k_lg64_shift forms
//     w <- w - S zhat in place (zhat is no basis vector, so the shift cannot sit on the diagonal); then the same two Gram-Schmidt
//     passes against v_0 .. v_j, the same decision and the same k_gm64_finish, which is handed a shift of 0 and so puts nothing on
//     the diagonal; v_{j+1} = w / |w|.  Inner target, steps_left and the |w| = 0 exit as ever.
//   Every step costs one product and `products` counts it (A zhat is not cached); n_aug counts the augmentation steps of a solve.
//   End of an augmented cycle: k_lg64_combine reads min(k, nk) basis rows and k - min(k, nk) ring entries (k = steps completed, on
//     the device), writes y and dy into the slot that is due and the partials of |dy|^2; k_lg64_norm (one block) turns them into
//     n, the stored flag and the ring's new head; k_gm64_scale divides the slot by n once the next head of a cycle has re-armed the
//     flag it is gated by (a solve that ends there needs no zhat).
//   The ring has (the handle's augment) + 1 slots: the slot that is due is never one of this cycle's sources, so the combine needs
//     no care about the order of its reads and its write.  psignn_gmres64_bytes counts the slots.
//   Stall ratio: the stagnation test is c > 0 && !(rel <= stall * prev_rel), 0 < stall <= 1; 0.5 is the rule above, 1.0 stops only
//     when a cycle does not lower rel at all; a NaN still stops there.
//   augment = 0, stall = 0.5 launches exactly the kernels of the plain solve, with its arguments, and gives its bits.
#include "f64_common.h"
#include "gmres_dense.h"
#include <math.h>

struct G64State {
  // the cycle (re-armed by k_ag64_check)
  int32_t k;            // Arnoldi steps completed
  int32_t done;         // the cycle is over (or the solve): every gated kernel returns
  int32_t reorth;       // this step's second Gram-Schmidt pass runs
  int32_t n_reorth;     // steps of this solve whose second pass ran
  // the solve
  int32_t cycles;       // restart cycles begun = entries of the traces
  int32_t products;     // transposed products spent
  int32_t solved;       // the solve is over
  int32_t stop;         // 0 budget, 1 tolerance, 2 stagnation
  int32_t steps_left;   // Arnoldi steps this cycle may take
  int32_t improved;     // this cycle's iterate has the lowest rel so far
  double beta;          // |f(y)| of the cycle: the inner target is |g| <= eps / 2 * beta
  double hn;            // |w| of the last step
  double n0sq;          // |w|^2 before the first pass of the current step
  double rnorm;         // |r| of the cycle
  double prev_rel, lowest, lowest_abs;
  // augmented restarts (all 0 in a plain solve)
  int32_t nk, ka;       // this cycle's plan: Krylov steps, augmentation steps (nk + ka = steps_left)
  int32_t stored;       // corrections in the ring
  int32_t head;         // the ring slot that is due
  int32_t n_aug;        // augmentation steps of this solve
  int32_t dy_ok;        // the last cycle's correction went into the ring (its slot still holds dy, not dy / n)
  double dyn;           // |dy| of the last cycle
};

struct psignn_gmres64 {
  psignn_f64_t* f = nullptr;   // borrowed
  int64_t N = 0, M = 0, nblk = 0, nchunk = 0;
  int m = 0;
  double* V = nullptr;      // (m + 1, M) basis
  double* vec = nullptr;    // 3 vectors of M: y, f(y), y_best
  double* part = nullptr;   // 2 planes of nblk block partials
  double* partD = nullptr;  // (m + 2, nchunk) dot partials
  double *coef = nullptr, *hcol = nullptr;   // (m + 2) each: this pass's coefficients; h1 + h2
  double *R = nullptr, *cs = nullptr, *sn = nullptr, *g = nullptr, *z = nullptr;   // (m + 1, m) column-major; (m + 1) each
  double *rel_trace = nullptr, *abs_trace = nullptr;   // (cap) device
  int cap = 0;
  int augment = 0;          // corrections a solve on this handle may keep
  double* Z = nullptr;      // (augment + 1, M) ring of corrections; NULL when augment = 0
  G64State* st = nullptr;     // device
  G64State* h_st = nullptr;   // pinned
};

// ------------------------------------------------------------------ the head of a cycle
__global__ void k_ag64_init(G64State* st) {
  G64State s{};
  *st = s;
}

// r = f(y) - y -> r0 (first: y <- 0, f(y) = grad); partials of |r|^2 and |f(y)|^2.  M is even: a lane's two elements are both
// inside or both outside.
// LIN, the shifted solve: fy holds the raw product A y, r = (A y + grad) - shift y, and the second partial is |grad|^2.
template <bool LIN>
__global__ void __launch_bounds__(F64_TB) k_ag64_begin(int64_t M, int64_t nblk, const G64State* __restrict__ st, double* __restrict__ y,
                                                       const double* __restrict__ fy, const double* __restrict__ grad, double shift,
                                                       double* __restrict__ r0, double* __restrict__ part, int first) {
  if (st->solved) return;
  __shared__ double sh[4];
  const int64_t e = ((int64_t)blockIdx.x * F64_TB + threadIdx.x) * 2;
  double sr = 0.0, sf = 0.0;
  if (e < M) {
    double2 f, a, r;
    if (first) {
      f = *(const double2*)(grad + e);
      a.x = 0.0;
      a.y = 0.0;
      *(double2*)(y + e) = a;
    } else {
      f = *(const double2*)(fy + e);
      a = *(const double2*)(y + e);
    }
    if (LIN) {
      const double2 b = *(const double2*)(grad + e);
      if (!first) {
        f.x += b.x;
        f.y += b.y;
      }
      r.x = fma(-shift, a.x, f.x);
      r.y = fma(-shift, a.y, f.y);
      f = b;
    } else {
      r.x = f.x - a.x;
      r.y = f.y - a.y;
    }
    *(double2*)(r0 + e) = r;
    sr = fma(r.y, r.y, r.x * r.x);
    sf = fma(f.y, f.y, f.x * f.x);
  }
  sr = f64_block_sum(sr, sh);
  sf = f64_block_sum(sf, sh);
  if (threadIdx.x == 0) {
    part[blockIdx.x] = sr;
    part[nblk + blockIdx.x] = sf;
  }
}

// LIN, the shifted solve: the linear measure rel = |r| / |b| (0 when r = 0), met at rel <= eps
// AUG, a solve with kept corrections or another stall ratio: the ratio is `stall`, the last cycle's augmentation steps are counted
// and the cycle's plan is written.  The plain solve (AUG false) compiles to what it always was.
template <bool LIN, bool AUG>
__device__ __forceinline__ void g64_check(G64State* st, const double* __restrict__ part, int64_t nblk, double* __restrict__ g,
                                          double* __restrict__ rel_trace, double* __restrict__ abs_trace, int cap, double eps,
                                          int max_products, int m, double stall, int augment) {
  if (st->solved) return;
  __shared__ double sh[4];
  const double sr = f64_final_sum(part, nblk, sh);
  const double sf = f64_final_sum(part + nblk, nblk, sh);
  if (threadIdx.x != 0) return;
  const double nr = sqrt(sr), nf = sqrt(sf);
  const double rel = LIN ? (nr == 0.0 ? 0.0 : nr / nf) : nr / (nf + 1e-9);
  const int c = st->cycles;
  const int products = st->products + (c > 0 ? st->k + 1 : 0);   // the last cycle's steps and this cycle's residual
  st->products = products;
  st->cycles = c + 1;
  if (c < cap) {
    rel_trace[c] = rel;
    abs_trace[c] = nr;
  }
  const int better = c == 0 || rel < st->lowest;
  st->improved = better;
  if (better) {
    st->lowest = rel;
    st->lowest_abs = nr;
  }
  const int left = min(m, max_products - products - 1);
  int done = 1, stop = 0;
  if ((LIN ? rel <= eps : rel < eps) || nr == 0.0) stop = 1;   // (a zero right-hand side: y = 0 is the answer)
  else if (c > 0 && !(rel <= (AUG ? stall : 0.5) * st->prev_rel)) stop = 2;   // (a NaN stops here too)
  else if (left <= 0) stop = 0;
  else done = 0;
  st->prev_rel = rel;
  st->solved = done;
  st->stop = stop;
  st->steps_left = done ? 0 : left;
  st->rnorm = nr;
  st->done = done;
  if (AUG && c > 0 && st->k > st->nk) st->n_aug += st->k - st->nk;
  if (!done) {
    if (AUG) {
      const int ka = lgm_plan_ka(st->stored, augment, left);
      st->ka = ka;
      st->nk = left - ka;
    }
    st->k = 0;
    st->reorth = 1;
    st->beta = nf;
    st->hn = 0.0;
    st->n0sq = 0.0;
    g[0] = nr;
  }
}
template <bool LIN>
__global__ void __launch_bounds__(F64_TB) k_ag64_check(G64State* st, const double* __restrict__ part, int64_t nblk,
                                                       double* __restrict__ g, double* __restrict__ rel_trace,
                                                       double* __restrict__ abs_trace, int cap, double eps, int max_products, int m) {
  g64_check<LIN, false>(st, part, nblk, g, rel_trace, abs_trace, cap, eps, max_products, m, 0.5, 0);
}
template <bool LIN>
__global__ void __launch_bounds__(F64_TB) k_lg64_check(G64State* st, const double* __restrict__ part, int64_t nblk,
                                                       double* __restrict__ g, double* __restrict__ rel_trace,
                                                       double* __restrict__ abs_trace, int cap, double eps, int max_products, int m,
                                                       double stall, int augment) {
  g64_check<LIN, true>(st, part, nblk, g, rel_trace, abs_trace, cap, eps, max_products, m, stall, augment);
}

// not gated by the flags: the cycle that ends the solve may be the lowest one
__global__ void __launch_bounds__(F64_TB) k_ag64_keep(int64_t M, const G64State* __restrict__ st, const double* __restrict__ y,
                                                      double* __restrict__ ybest) {
  if (!st->improved) return;
  const int64_t e = ((int64_t)blockIdx.x * F64_TB + threadIdx.x) * 2;
  if (e < M) *(double2*)(ybest + e) = *(const double2*)(y + e);
}

// dst = src / *scale (|r| or |w|, a device double)
__global__ void __launch_bounds__(F64_TB) k_gm64_scale(int64_t M, const G64State* __restrict__ st, const double* __restrict__ src,
                                                       const double* __restrict__ scale, double* __restrict__ dst) {
  if (st->done) return;
  const int64_t e = ((int64_t)blockIdx.x * F64_TB + threadIdx.x) * 2;
  if (e >= M) return;
  const double s = *scale;
  double2 v = *(const double2*)(src + e);
  v.x /= s;
  v.y /= s;
  *(double2*)(dst + e) = v;
}

// ------------------------------------------------------------------ one Arnoldi step
// Block = chunk of F64_CHUNK elements of w in LDS; wave q takes rows q, q + 4, ... of the `rows` first basis rows (row j + 1 is w
// itself: |w|^2 in the first pass).  A lane reads 8 double2 of the row (index (i * 64 + lane) * 2 within the chunk).
// partD[row * nchunk + chunk].
template <bool FULL>
__device__ __forceinline__ void g64_dots_chunk(int64_t M, int64_t nchunk, int rows, const double* __restrict__ V,
                                               const double* __restrict__ w, double* __restrict__ partD, double2* s_w) {
  const int64_t base = (int64_t)blockIdx.x * F64_CHUNK;
  for (int i = threadIdx.x; i < F64_CHUNK / 2; i += F64_TB) s_w[i] = f64_ld2<FULL>(w, base + 2 * i, base, M);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll 1
  for (int r = wave; r < rows; r += F64_TB / 64) {
    const double* Vr = V + (int64_t)r * M;
    double2 v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = f64_ld2<FULL>(Vr, base + (int64_t)(i * 64 + lane) * 2, base, M);
    double a = 0.0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const double2 x = s_w[i * 64 + lane];
      a = fma(v[i].x, x.x, a);
      a = fma(v[i].y, x.y, a);
    }
    a = f64_wave_sum(a);
    if (lane == 0) partD[(int64_t)r * nchunk + blockIdx.x] = a;
  }
}
__global__ void __launch_bounds__(F64_TB) k_gm64_dots(int64_t M, int64_t nchunk, int j, int pass, const G64State* __restrict__ st,
                                                      const double* __restrict__ V, double* __restrict__ partD) {
  if (st->done || (pass && !st->reorth)) return;
  __shared__ double2 s_w[F64_CHUNK / 2];
  const double* w = V + (int64_t)(j + 1) * M;
  const int rows = j + 1 + (pass == 0);
  if (((int64_t)blockIdx.x + 1) * F64_CHUNK <= M) g64_dots_chunk<true>(M, nchunk, rows, V, w, partD, s_w);
  else g64_dots_chunk<false>(M, nchunk, rows, V, w, partD, s_w);
}

// one block per coefficient: pass 1 h_i (and |w|^2 from row j + 1), pass 2 the correction, added to h_i
__global__ void __launch_bounds__(F64_TB) k_gm64_reduce(int64_t nchunk, int j, int pass, G64State* __restrict__ st,
                                                        const double* __restrict__ partD, double* __restrict__ coef,
                                                        double* __restrict__ hcol) {
  if (st->done || (pass && !st->reorth)) return;
  __shared__ double sh[4];
  const int r = blockIdx.x;
  const double s = f64_final_sum(partD + (int64_t)r * nchunk, nchunk, sh);
  if (threadIdx.x != 0) return;
  if (r == j + 1) {
    st->n0sq = s;
  } else {
    coef[r] = s;
    hcol[r] = pass ? hcol[r] + s : s;
  }
}

// w -= sum_{i <= j} coef_i v_i, two elements per lane, rows in ascending order; block partials of |w'|^2
__global__ void __launch_bounds__(F64_TB) k_gm64_axpy(int64_t M, int j, int pass, const G64State* __restrict__ st,
                                                      double* __restrict__ V, const double* __restrict__ coef,
                                                      double* __restrict__ part) {
  if (st->done || (pass && !st->reorth)) return;
  __shared__ double sh[4];
  const int64_t e = ((int64_t)blockIdx.x * F64_TB + threadIdx.x) * 2;
  double s = 0.0;
  if (e < M) {
    double2 acc = {0.0, 0.0};
#pragma unroll 4
    for (int i = 0; i <= j; ++i) {
      const double c = coef[i];
      const double2 v = *(const double2*)(V + (int64_t)i * M + e);
      acc.x = fma(c, v.x, acc.x);
      acc.y = fma(c, v.y, acc.y);
    }
    double* w = V + (int64_t)(j + 1) * M + e;
    double2 x = *(const double2*)w;
    x.x -= acc.x;
    x.y -= acc.y;
    *(double2*)w = x;
    s = fma(x.y, x.y, x.x * x.x);
  }
  s = f64_block_sum(s, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

__global__ void __launch_bounds__(F64_TB) k_gm64_decide(G64State* st, const double* __restrict__ part, int64_t nblk) {
  if (st->done) return;
  __shared__ double sh[4];
  const double s = f64_final_sum(part, nblk, sh);
  if (threadIdx.x != 0) return;
  const int r = !(s >= 0.5 * st->n0sq);
  st->reorth = r;
  st->n_reorth += r;
}

// One block: column j of the Hessenberg matrix and the least-squares update.  `part` holds |w|^2 of the last pass that ran.
__global__ void __launch_bounds__(F64_TB) k_gm64_finish(G64State* st, const double* __restrict__ part, int64_t nblk, int j, int m,
                                                        double eta, double shift, double* __restrict__ hcol, double* __restrict__ R,
                                                        double* __restrict__ cs, double* __restrict__ sn, double* __restrict__ g) {
  if (st->done) return;
  __shared__ double sh[4];
  const double s2 = f64_final_sum(part, nblk, sh);
  if (threadIdx.x != 0) return;
  const double hn = sqrt(s2);
  st->hn = hn;
  hcol[j] -= shift;   // Hessenberg of A - shift I from the Arnoldi relation of A (the adjoint solve: shift = 1)
  hcol[j + 1] = hn;
  const double resid = gmd_column(j, hcol, cs, sn, g);
  double* col = R + (int64_t)j * (m + 1);
  for (int i = 0; i <= j; ++i) col[i] = hcol[i];
  st->k = j + 1;
  st->reorth = 1;
  if (resid <= eta * st->beta || j + 1 >= st->steps_left || !(hn > 0.0)) st->done = 1;
}

// ------------------------------------------------------------------ the end of a cycle (not gated: the cycle's flag is up)
__global__ void k_gm64_backsolve(const G64State* __restrict__ st, int m, const double* __restrict__ R, const double* __restrict__ g,
                                 double* __restrict__ z) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  gmd_backsolve(st->k, m + 1, R, g, z);
}
// y -= sum_{i < k} z_i v_i
__global__ void __launch_bounds__(F64_TB) k_gm64_combine(int64_t M, const G64State* __restrict__ st, const double* __restrict__ V,
                                                         const double* __restrict__ z, double* __restrict__ y) {
  const int64_t e = ((int64_t)blockIdx.x * F64_TB + threadIdx.x) * 2;
  if (e >= M) return;
  const int k = st->k;
  double2 acc = {0.0, 0.0};
#pragma unroll 4
  for (int i = 0; i < k; ++i) {
    const double c = z[i];
    const double2 v = *(const double2*)(V + (int64_t)i * M + e);
    acc.x = fma(c, v.x, acc.x);
    acc.y = fma(c, v.y, acc.y);
  }
  double2 x = *(const double2*)(y + e);
  x.x -= acc.x;
  x.y -= acc.y;
  *(double2*)(y + e) = x;
}

// ------------------------------------------------------------------ augmented restarts
// w -= S zhat in place, the head of an augmentation step: two reads, one write, 16 bytes per lane
__global__ void __launch_bounds__(F64_TB) k_lg64_shift(int64_t M, const G64State* __restrict__ st, const double* __restrict__ zhat,
                                                       double S, double* __restrict__ w) {
  if (st->done) return;
  const int64_t e = ((int64_t)blockIdx.x * F64_TB + threadIdx.x) * 2;
  if (e >= M) return;
  const double2 z = *(const double2*)(zhat + e);
  double2 x = *(const double2*)(w + e);
  x.x = fma(-S, z.x, x.x);
  x.y = fma(-S, z.y, x.y);
  *(double2*)(w + e) = x;
}
// The end of an augmented cycle (not gated: the cycle's flag is up): dy = sum_{i < min(k, nk)} z_i v_i + sum_{nk <= i < k} z_i
// zhat_(i - nk), the basis rows first, each list in ascending order; y -= dy; dy -> the ring slot that is due (never a source: the
// ring has one slot more than a cycle reads); block partials of |dy|^2.  Each source is read once, 16 bytes per lane.
__global__ void __launch_bounds__(F64_TB) k_lg64_combine(int64_t M, const G64State* __restrict__ st, const double* __restrict__ V,
                                                         double* Z /* read and written: distinct slots */, int nslots,
                                                         const double* __restrict__ z, double* __restrict__ y,
                                                         double* __restrict__ part) {
  __shared__ double sh[4];
  const int64_t e = ((int64_t)blockIdx.x * F64_TB + threadIdx.x) * 2;
  const int k = st->k, nk = st->nk, head = st->head;
  const int kb = k < nk ? k : nk;
  double s = 0.0;
  if (e < M) {
    double2 acc = {0.0, 0.0};
#pragma unroll 4
    for (int i = 0; i < kb; ++i) {
      const double c = z[i];
      const double2 v = *(const double2*)(V + (int64_t)i * M + e);
      acc.x = fma(c, v.x, acc.x);
      acc.y = fma(c, v.y, acc.y);
    }
    for (int i = nk; i < k; ++i) {
      const double c = z[i];
      const double2 v = *(const double2*)(Z + (int64_t)lgm_slot_newest(head, nslots, i - nk) * M + e);
      acc.x = fma(c, v.x, acc.x);
      acc.y = fma(c, v.y, acc.y);
    }
    double2 x = *(const double2*)(y + e);
    x.x -= acc.x;
    x.y -= acc.y;
    *(double2*)(y + e) = x;
    *(double2*)(Z + (int64_t)lgm_slot_due(head) * M + e) = acc;
    s = fma(acc.y, acc.y, acc.x * acc.x);
  }
  s = f64_block_sum(s, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}
// One block: n = |dy|; when n > 0 and finite the slot that was due becomes the newest entry (it holds dy until the next head of a
// cycle divides it by n) and the `augment` newest are kept.
__global__ void __launch_bounds__(F64_TB) k_lg64_norm(G64State* st, const double* __restrict__ part, int64_t nblk, int nslots,
                                                      int augment) {
  __shared__ double sh[4];
  const double s2 = f64_final_sum(part, nblk, sh);
  if (threadIdx.x != 0) return;
  const double n = sqrt(s2);
  const int ok = n > 0.0 && n < INFINITY;   // (a NaN is neither)
  st->dyn = n;
  st->dy_ok = ok;
  if (ok) {
    st->head = lgm_push(st->head, nslots);
    st->stored = lgm_stored_after_push(st->stored, augment);
  }
}

// ------------------------------------------------------------------ the vector kernels of the Newton loop (newton_f64.hip)
// g = f(x) - x; partials of |g|^2 and |f(x)|^2.  M is even: a lane's two elements are both inside or both outside.
__global__ void __launch_bounds__(F64_TB) k_nt64_resid(int64_t M, int64_t nblk, const double* __restrict__ fx,
                                                       const double* __restrict__ x, double* __restrict__ g,
                                                       double* __restrict__ part) {
  __shared__ double sh[4];
  const int64_t e = ((int64_t)blockIdx.x * F64_TB + threadIdx.x) * 2;
  double sg = 0.0, sf = 0.0;
  if (e < M) {
    const double2 f = *(const double2*)(fx + e), a = *(const double2*)(x + e);
    double2 r;
    r.x = f.x - a.x;
    r.y = f.y - a.y;
    *(double2*)(g + e) = r;
    sg = fma(r.y, r.y, r.x * r.x);
    sf = fma(f.y, f.y, f.x * f.x);
  }
  sg = f64_block_sum(sg, sh);
  sf = f64_block_sum(sf, sh);
  if (threadIdx.x == 0) {
    part[blockIdx.x] = sg;
    part[nblk + blockIdx.x] = sf;
  }
}

__global__ void __launch_bounds__(F64_TB) k_nt64_norms(const double* __restrict__ part, int64_t nblk, double* __restrict__ norms) {
  __shared__ double sh[4];
  const double sg = f64_final_sum(part, nblk, sh);
  const double sf = f64_final_sum(part + nblk, nblk, sh);
  if (threadIdx.x == 0) {
    norms[0] = sqrt(sg);
    norms[1] = sqrt(sf);
  }
}

__global__ void __launch_bounds__(F64_TB) k_nt64_add(int64_t M, const double* __restrict__ x, const double* __restrict__ d,
                                                     double* __restrict__ xt) {
  const int64_t e = ((int64_t)blockIdx.x * F64_TB + threadIdx.x) * 2;
  if (e >= M) return;
  const double2 a = *(const double2*)(x + e), b = *(const double2*)(d + e);
  double2 r;
  r.x = a.x + b.x;
  r.y = a.y + b.y;
  *(double2*)(xt + e) = r;
}

// (internal.h) block partials of a vector of M doubles; g = fx - x with |g| and |fx| into norms[0 .. 1]; xt = x + d
int64_t psignn_nt64_blocks(int64_t M) { return cdiv(M, 2 * F64_TB); }
void psignn_nt64_resid_norms(int64_t M, const double* fx, const double* x, double* g, double* part, double* norms, hipStream_t st) {
  const int64_t nblk = psignn_nt64_blocks(M);
  PROF_BYTES(3 * M * 8);
  LAUNCH("k_nt64_resid", st, (k_nt64_resid<<<(unsigned)nblk, F64_TB, 0, st>>>(M, nblk, fx, x, g, part)));
  LAUNCH("k_nt64_norms", st, (k_nt64_norms<<<1, F64_TB, 0, st>>>(part, nblk, norms)));
}
void psignn_nt64_add(int64_t M, const double* x, const double* d, double* xt, hipStream_t st) {
  PROF_BYTES(3 * M * 8);
  LAUNCH("k_nt64_add", st, (k_nt64_add<<<(unsigned)psignn_nt64_blocks(M), F64_TB, 0, st>>>(M, x, d, xt)));
}

// ------------------------------------------------------------------ host
extern "C" void psignn_gmres64_destroy(psignn_gmres64_t* s) {
  if (!s) return;
  void* ptrs[] = {s->V, s->vec, s->part, s->partD, s->coef, s->hcol, s->R, s->cs, s->sn, s->g, s->z, s->rel_trace, s->abs_trace, s->st, s->Z};
  for (void* q : ptrs)
    if (q) (void)hipFree(q);
  if (s->h_st) (void)hipHostFree(s->h_st);
  delete s;
}

static int g64_create(const char* who, psignn_gmres64_t** out, psignn_f64_t* f, int m, int augment) {
  ARG_CHECK_AS(who, out != nullptr, "out is NULL");
  *out = nullptr;
  ARG_CHECK_AS(who, f != nullptr, "the float64 map handle is NULL");
  ARG_CHECK_AS(who, m >= 1 && m <= 4096, "restart length out of range (1 .. 4096)");
  ARG_CHECK_AS(who, augment >= 0 && augment <= 8 && augment <= m - 1, "augment out of range (0 .. min(m - 1, 8))");
  const psignn_plan* p = psignn_f64_plan(f);
  ARG_CHECK_AS(who, p->N > 0, "the plan has no nodes");
  psignn_gmres64* s = new psignn_gmres64();
  s->f = f;
  s->N = p->N;
  s->M = p->N * D;
  s->m = m;
  s->nblk = cdiv(s->M, 2 * F64_TB);
  s->nchunk = cdiv(s->M, F64_CHUNK);
  const size_t basis_bytes = (size_t)(m + 1) * (size_t)s->M * sizeof(double);
  if (hipMalloc((void**)&s->V, basis_bytes) != hipSuccess) {
    (void)hipGetLastError();   // the failed allocation is reported here, not by the next launch
    s->V = nullptr;
    psignn_set_error("%s: cannot allocate the float64 basis: (m + 1) * N * d * 8 = %d * %lld * %d * 8 = %zu bytes", who, m + 1,
                     (long long)s->N, D, basis_bytes);
    psignn_gmres64_destroy(s);
    return PSIGNN_ENOMEM;
  }
  const size_t ring_bytes = augment ? (size_t)(augment + 1) * (size_t)s->M * sizeof(double) : 0;
  if (ring_bytes && hipMalloc((void**)&s->Z, ring_bytes) != hipSuccess) {
    (void)hipGetLastError();
    s->Z = nullptr;
    psignn_set_error("%s: cannot allocate the ring of corrections: (augment + 1) * N * d * 8 = %d * %lld * %d * 8 = %zu bytes", who,
                     augment + 1, (long long)s->N, D, ring_bytes);
    psignn_gmres64_destroy(s);
    return PSIGNN_ENOMEM;
  }
  s->augment = augment;
  auto fail = [&](int code) {
    psignn_gmres64_destroy(s);
    return code;
  };
  HIP_TRY_OR(hipMalloc((void**)&s->vec, (size_t)3 * s->M * sizeof(double)), fail(PSIGNN_EHIP));
  HIP_TRY_OR(hipMalloc((void**)&s->part, (size_t)2 * s->nblk * sizeof(double)), fail(PSIGNN_EHIP));
  HIP_TRY_OR(hipMalloc((void**)&s->partD, (size_t)(m + 2) * s->nchunk * sizeof(double)), fail(PSIGNN_EHIP));
  HIP_TRY_OR(hipMalloc((void**)&s->coef, (size_t)(m + 2) * sizeof(double)), fail(PSIGNN_EHIP));
  HIP_TRY_OR(hipMalloc((void**)&s->hcol, (size_t)(m + 2) * sizeof(double)), fail(PSIGNN_EHIP));
  HIP_TRY_OR(hipMalloc((void**)&s->R, (size_t)(m + 1) * m * sizeof(double)), fail(PSIGNN_EHIP));
  HIP_TRY_OR(hipMalloc((void**)&s->cs, (size_t)(m + 1) * sizeof(double)), fail(PSIGNN_EHIP));
  HIP_TRY_OR(hipMalloc((void**)&s->sn, (size_t)(m + 1) * sizeof(double)), fail(PSIGNN_EHIP));
  HIP_TRY_OR(hipMalloc((void**)&s->g, (size_t)(m + 1) * sizeof(double)), fail(PSIGNN_EHIP));
  HIP_TRY_OR(hipMalloc((void**)&s->z, (size_t)(m + 1) * sizeof(double)), fail(PSIGNN_EHIP));
  HIP_TRY_OR(hipMalloc((void**)&s->st, sizeof(G64State)), fail(PSIGNN_EHIP));
  HIP_TRY_OR(hipHostMalloc((void**)&s->h_st, sizeof(G64State)), fail(PSIGNN_EHIP));
  *out = s;
  return PSIGNN_OK;
}
extern "C" int psignn_gmres64_create(psignn_gmres64_t** out, psignn_f64_t* f, int m) { return g64_create(__func__, out, f, m, 0); }
extern "C" int psignn_gmres64_create_aug(psignn_gmres64_t** out, psignn_f64_t* f, int m, int augment) {
  return g64_create(__func__, out, f, m, augment);
}

int psignn_gmres64_augment(const psignn_gmres64_t* s) { return s ? s->augment : 0; }   // (internal.h)

extern "C" size_t psignn_gmres64_bytes(const psignn_gmres64_t* s) {
  if (!s) return 0;
  const size_t m = (size_t)s->m;
  return ((m + 1) + 3 + (s->augment ? (size_t)s->augment + 1 : 0)) * (size_t)s->M * sizeof(double) +
         ((size_t)2 * s->nblk + (m + 2) * (size_t)s->nchunk + 2 * (m + 2) + (m + 1) * m + 4 * (m + 1) + 2 * (size_t)s->cap) * sizeof(double) +
         sizeof(G64State);
}

// the traces hold one entry per cycle; a cycle after the first spends at least two products
static int g64_traces(psignn_gmres64* s, int max_products) {
  const int cap = max_products / 2 + 3;
  if (s->cap >= cap) return PSIGNN_OK;
  if (s->rel_trace) (void)hipFree(s->rel_trace);
  if (s->abs_trace) (void)hipFree(s->abs_trace);
  s->rel_trace = s->abs_trace = nullptr;
  s->cap = 0;
  HIP_TRY(hipMalloc((void**)&s->rel_trace, (size_t)cap * sizeof(double)));
  HIP_TRY(hipMalloc((void**)&s->abs_trace, (size_t)cap * sizeof(double)));
  s->cap = cap;
  return PSIGNN_OK;
}

// One solve on the handle.  LIN = false: the adjoint system y = J^T y + grad with Broyden's measure (shift 1, transposed).
// LIN = true: shift * y = A y + grad with the linear measure, A = J (transposed = 0) or J^T; the residual's product is then the raw
// one and k_ag64_begin adds grad.  The launches of the adjoint solve are those it has always made.
template <bool LIN>
static int g64_solve(const char* who, psignn_gmres64* s, const double* W, int nl, const double* h_star, const double* h0,
                     const double* prb, const double* nrm, const double* grad, double shift, int transposed, double eps,
                     int max_products, int poll_every, const psignn_gmres64_opts_t& o, double* work, int64_t work_doubles,
                     double* result, psignn_gmres64_info_t* h_info, double* h_rel_trace, double* h_abs_trace, hipStream_t st) {
  ARG_CHECK_AS(who, o.augment >= 0 && o.augment <= s->augment, "augment out of range (0 .. the handle's augment)");
  ARG_CHECK_AS(who, o.stall > 0.0 && o.stall <= 1.0, "stall must be in (0, 1]");   // (a NaN is not)
  const int aug = o.augment, nslots = s->augment + 1;
  const bool plain = aug == 0 && o.stall == 0.5;   // the launches of the solve without options
  if (poll_every <= 0) poll_every = 8;
  int rc;
  if ((rc = g64_traces(s, max_products))) return rc;
  const int64_t M = s->M, nblk = s->nblk;
  const int m = s->m;
  const unsigned g2 = (unsigned)nblk, gc = (unsigned)s->nchunk;
  double *y = s->vec, *fy = s->vec + M, *ybest = s->vec + 2 * M;
  const int32_t* cycle_done = &s->st->done;
  auto product = [&](const double* x, const double* add, double* out, const int32_t* done) {
    if (transposed) return psignn_f64_vjp_gated(s->f, W, nl, h_star, h0, prb, nrm, x, add, out, work, work_doubles, done, st);
    return psignn_f64_jvp_gated(s->f, W, nl, h_star, h0, prb, nrm, x, out, work, work_doubles, done, st);
  };
  k_ag64_init<<<1, 1, 0, st>>>(s->st);
  for (int cycle = 0;; ++cycle) {
    // the residual's product is not gated: the flag of the cycle that just ended is still up
    if (cycle > 0 && (rc = product(y, LIN ? nullptr : grad, fy, nullptr))) return rc;
    PROF_BYTES((3 + LIN) * M * 8);
    LAUNCH("k_ag64_begin", st, (k_ag64_begin<LIN><<<g2, F64_TB, 0, st>>>(M, nblk, s->st, y, fy, grad, shift, s->V, s->part, cycle == 0)));
    if (plain)
      LAUNCH("k_ag64_check", st, (k_ag64_check<LIN><<<1, F64_TB, 0, st>>>(s->st, s->part, nblk, s->g, s->rel_trace, s->abs_trace, s->cap,
                                                                         eps, max_products, m)));
    else
      LAUNCH("k_lg64_check", st, (k_lg64_check<LIN><<<1, F64_TB, 0, st>>>(s->st, s->part, nblk, s->g, s->rel_trace, s->abs_trace, s->cap,
                                                                         eps, max_products, m, o.stall, aug)));
    PROF_BYTES(2 * M * 8);
    LAUNCH("k_ag64_keep", st, (k_ag64_keep<<<g2, F64_TB, 0, st>>>(M, s->st, y, ybest)));
    PROF_BYTES(2 * M * 8);
    LAUNCH("k_gm64_scale", st, (k_gm64_scale<<<g2, F64_TB, 0, st>>>(M, s->st, s->V, &s->st->rnorm, s->V)));
    HIP_TRY(hipMemcpyAsync(s->h_st, s->st, sizeof(G64State), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (s->h_st->solved) break;
    const int steps = s->h_st->steps_left;
    if (steps < 1 || steps > m) {
      psignn_set_error("%s: internal: %d Arnoldi steps allowed, restart length %d", who, steps, m);
      return PSIGNN_EHIP;
    }
    // the cycle's plan and the ring as the head of the cycle left them (a plain solve: all Krylov steps)
    const int nk = aug ? s->h_st->nk : steps, head = s->h_st->head;
    if (nk < 1 || nk > steps || steps - nk > aug || head < 0 || head >= nslots) {
      psignn_set_error("%s: internal: plan of %d Krylov steps out of %d, %d kept, ring head %d of %d", who, nk, steps, aug, head, nslots);
      return PSIGNN_EHIP;
    }
    if (aug && cycle > 0 && s->h_st->dy_ok) {   // zhat = dy / |dy|: the newest slot still holds the last cycle's dy
      double* zn = s->Z + (size_t)lgm_slot_newest(head, nslots, 0) * M;
      PROF_BYTES(2 * M * 8);
      LAUNCH("k_gm64_scale", st, (k_gm64_scale<<<g2, F64_TB, 0, st>>>(M, s->st, zn, &s->st->dyn, zn)));
    }
    for (int j = 0; j < steps; ++j) {
      double* w = s->V + (size_t)(j + 1) * M;
      const double* src = j < nk ? s->V + (size_t)j * M : s->Z + (size_t)lgm_slot_newest(head, nslots, j - nk) * M;
      if ((rc = product(src, nullptr, w, cycle_done))) return rc;
      if (j >= nk) {
        PROF_BYTES(3 * M * 8);
        LAUNCH("k_lg64_shift", st, (k_lg64_shift<<<g2, F64_TB, 0, st>>>(M, s->st, src, shift, w)));
      }
      for (int pass = 0; pass < 2; ++pass) {
        PROF_BYTES(((int64_t)j + 2 + (pass == 0)) * M * 8);
        LAUNCH("k_gm64_dots", st, (k_gm64_dots<<<gc, F64_TB, 0, st>>>(M, s->nchunk, j, pass, s->st, s->V, s->partD)));
        LAUNCH("k_gm64_reduce", st, (k_gm64_reduce<<<(unsigned)(j + 1 + (pass == 0)), F64_TB, 0, st>>>(s->nchunk, j, pass, s->st, s->partD,
                                                                                                      s->coef, s->hcol)));
        PROF_BYTES(((int64_t)j + 3) * M * 8);
        LAUNCH("k_gm64_axpy", st, (k_gm64_axpy<<<g2, F64_TB, 0, st>>>(M, j, pass, s->st, s->V, s->coef, s->part)));
        if (pass == 0) LAUNCH("k_gm64_decide", st, (k_gm64_decide<<<1, F64_TB, 0, st>>>(s->st, s->part, nblk)));
      }
      LAUNCH("k_gm64_finish", st, (k_gm64_finish<<<1, F64_TB, 0, st>>>(s->st, s->part, nblk, j, m, LIN ? eps : 0.5 * eps,
                                                                      j < nk ? shift : 0.0, s->hcol, s->R, s->cs, s->sn, s->g)));
      PROF_BYTES(2 * M * 8);
      LAUNCH("k_gm64_scale", st, (k_gm64_scale<<<g2, F64_TB, 0, st>>>(M, s->st, w, &s->st->hn, w)));
      if ((j + 1) % poll_every == 0 && j + 1 < steps) {
        HIP_TRY(hipMemcpyAsync(s->h_st, s->st, sizeof(G64State), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (s->h_st->done) break;
      }
    }
    LAUNCH("k_gm64_backsolve", st, (k_gm64_backsolve<<<1, 64, 0, st>>>(s->st, m, s->R, s->g, s->z)));
    if (!aug) {
      PROF_BYTES(((int64_t)m + 2) * M * 8);
      LAUNCH("k_gm64_combine", st, (k_gm64_combine<<<g2, F64_TB, 0, st>>>(M, s->st, s->V, s->z, y)));
    } else {
      PROF_BYTES(((int64_t)steps + 3) * M * 8);
      LAUNCH("k_lg64_combine", st, (k_lg64_combine<<<g2, F64_TB, 0, st>>>(M, s->st, s->V, s->Z, nslots, s->z, y, s->part)));
      LAUNCH("k_lg64_norm", st, (k_lg64_norm<<<1, F64_TB, 0, st>>>(s->st, s->part, nblk, nslots, aug)));
    }
  }
  HIP_TRY(hipGetLastError());
  const G64State& h = *s->h_st;
  if (h.cycles < 1 || h.products < 0 || h.products > max_products) {
    psignn_set_error("%s: internal: %d cycles, %d products recorded, budget %d", who, h.cycles, h.products, max_products);
    return PSIGNN_EHIP;
  }
  const int n = h.cycles < s->cap ? h.cycles : s->cap;
  HIP_TRY(hipMemcpyAsync(result, ybest, (size_t)M * sizeof(double), hipMemcpyDeviceToDevice, st));
  if (h_rel_trace) HIP_TRY(hipMemcpyAsync(h_rel_trace, s->rel_trace, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
  if (h_abs_trace) HIP_TRY(hipMemcpyAsync(h_abs_trace, s->abs_trace, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  h_info->products = h.products;
  h_info->cycles = h.cycles;
  h_info->stop_reason = h.stop;
  h_info->n_reorth = h.n_reorth;
  h_info->lowest = h.lowest;
  h_info->lowest_abs = h.lowest_abs;
  h_info->n_aug = h.n_aug;
  return PSIGNN_OK;
}
static const psignn_gmres64_opts_t G64_PLAIN = {0, 0.5};
static void g64_plain_info(const psignn_gmres64_info_t& i, psignn_gmres_adjoint_info_t* o) {
  o->products = i.products;
  o->cycles = i.cycles;
  o->stop_reason = i.stop_reason;
  o->n_reorth = i.n_reorth;
  o->lowest = i.lowest;
  o->lowest_abs = i.lowest_abs;
}

static int g64_adjoint(const char* who, psignn_gmres64_t* s, const double* W, int nl, const double* h_star, const double* h0,
                       const double* prb, const double* nrm, const double* grad, double eps, int max_products, int poll_every,
                       const psignn_gmres64_opts_t* o, double* work, int64_t work_doubles, double* result, psignn_gmres64_info_t* info,
                       double* h_rel_trace, double* h_abs_trace, void* stream) {
  ARG_CHECK_AS(who, s && W && h_star && h0 && prb && grad && work && result && o && info, "NULL argument");
  ARG_CHECK_AS(who, nl >= 1 && nl <= 64, "n_layers out of range");
  ARG_CHECK_AS(who, eps >= 0.0 && eps < INFINITY, "eps must be finite and >= 0");
  ARG_CHECK_AS(who, max_products >= 1 && max_products <= (1 << 24), "max_products out of range");
  return g64_solve<false>(who, s, W, nl, h_star, h0, prb, nrm, grad, 1.0, 1, eps, max_products, poll_every, *o, work, work_doubles, result,
                          info, h_rel_trace, h_abs_trace, (hipStream_t)stream);
}
extern "C" int psignn_gmres64_solve_adjoint(psignn_gmres64_t* s, const double* W, int nl, const double* h_star, const double* h0,
                                            const double* prb, const double* nrm, const double* grad, double eps, int max_products,
                                            int poll_every, double* work, int64_t work_doubles, double* result,
                                            psignn_gmres_adjoint_info_t* h_info, double* h_rel_trace, double* h_abs_trace,
                                            void* stream) {
  ARG_CHECK(h_info != nullptr, "NULL argument");
  psignn_gmres64_info_t info;
  const int rc = g64_adjoint(__func__, s, W, nl, h_star, h0, prb, nrm, grad, eps, max_products, poll_every, &G64_PLAIN, work, work_doubles,
                             result, &info, h_rel_trace, h_abs_trace, stream);
  if (rc == PSIGNN_OK) g64_plain_info(info, h_info);
  return rc;
}
extern "C" int psignn_gmres64_solve_adjoint_opts(psignn_gmres64_t* s, const double* W, int nl, const double* h_star, const double* h0,
                                                 const double* prb, const double* nrm, const double* grad, double eps,
                                                 int max_products, int poll_every, const psignn_gmres64_opts_t* opts, double* work,
                                                 int64_t work_doubles, double* result, psignn_gmres64_info_t* h_info,
                                                 double* h_rel_trace, double* h_abs_trace, void* stream) {
  return g64_adjoint(__func__, s, W, nl, h_star, h0, prb, nrm, grad, eps, max_products, poll_every, opts, work, work_doubles, result,
                     h_info, h_rel_trace, h_abs_trace, stream);
}

// The shifted linear solve shift * delta = A delta + b from delta = 0, A = J_f(h) (transposed = 0) or J_f(h)^T: the linear system of
// a Newton step on g(x) = f(x) - x with a pseudo-transient shift, (1 + sigma) delta = J delta + g (newton_f64.hip), and its dual.
// The handle, the basis, the kernels and the cycle structure of the adjoint solve; the shift on the Hessenberg's diagonal, the
// residual r = A delta + b - shift * delta, the linear measure rel = |r| / |b| with rel <= eta as the tolerance and |g_{j+1}| <=
// eta * |b| as the inner target (an inexact Newton step asks for no more; the head of the next cycle confirms it on the true residual).  The workspace is the larger of the two products'.
static int g64_shifted(const char* who, psignn_gmres64_t* s, const double* W, int nl, const double* h, const double* h0,
                       const double* prb, const double* nrm, const double* b, double shift, int transposed, double eta,
                       int max_products, int poll_every, const psignn_gmres64_opts_t* o, double* work, int64_t work_doubles,
                       double* result, psignn_gmres64_info_t* info, double* h_rel_trace, double* h_abs_trace, void* stream) {
  ARG_CHECK_AS(who, s && W && h && h0 && prb && b && result && o && info, "NULL argument");
  ARG_CHECK_AS(who, nl >= 1 && nl <= 64, "n_layers out of range");
  ARG_CHECK_AS(who, shift >= 1.0 && shift < INFINITY, "shift must be finite and >= 1");
  ARG_CHECK_AS(who, eta >= 0.0 && eta < INFINITY, "eta must be finite and >= 0");
  ARG_CHECK_AS(who, max_products >= 1 && max_products <= (1 << 24), "max_products out of range");
  ARG_CHECK_AS(who, result != h && result != b, "result must not alias h or b");
  const int64_t need = ws::shifted64_total(psignn_f64_deriv_workspace_doubles(s->f, nl, 0), psignn_f64_deriv_workspace_doubles(s->f, nl, 1));
  if (need > 0 && (!work || work_doubles < need)) {
    psignn_set_error("%s: the workspace holds %lld doubles, %lld are needed (%lld bytes)", who, (long long)(work ? work_doubles : 0),
                     (long long)need, (long long)need * 8);
    return PSIGNN_ENOMEM;
  }
  return g64_solve<true>(who, s, W, nl, h, h0, prb, nrm, b, shift, transposed != 0, eta, max_products, poll_every, *o, work, work_doubles,
                         result, info, h_rel_trace, h_abs_trace, (hipStream_t)stream);
}
extern "C" int psignn_gmres64_solve_shifted(psignn_gmres64_t* s, const double* W, int nl, const double* h, const double* h0,
                                            const double* prb, const double* nrm, const double* b, double shift, int transposed,
                                            double eta, int max_products, int poll_every, double* work, int64_t work_doubles,
                                            double* result, psignn_gmres_adjoint_info_t* h_info, double* h_rel_trace,
                                            double* h_abs_trace, void* stream) {
  ARG_CHECK(h_info != nullptr, "NULL argument");
  psignn_gmres64_info_t info;
  const int rc = g64_shifted(__func__, s, W, nl, h, h0, prb, nrm, b, shift, transposed, eta, max_products, poll_every, &G64_PLAIN, work,
                             work_doubles, result, &info, h_rel_trace, h_abs_trace, stream);
  if (rc == PSIGNN_OK) g64_plain_info(info, h_info);
  return rc;
}
extern "C" int psignn_gmres64_solve_shifted_opts(psignn_gmres64_t* s, const double* W, int nl, const double* h, const double* h0,
                                                 const double* prb, const double* nrm, const double* b, double shift, int transposed,
                                                 double eta, int max_products, int poll_every, const psignn_gmres64_opts_t* opts,
                                                 double* work, int64_t work_doubles, double* result, psignn_gmres64_info_t* h_info,
                                                 double* h_rel_trace, double* h_abs_trace, void* stream) {
  return g64_shifted(__func__, s, W, nl, h, h0, prb, nrm, b, shift, transposed, eta, max_products, poll_every, opts, work, work_doubles,
                     result, h_info, h_rel_trace, h_abs_trace, stream);
}
