// Broyden root-find of g(x) = f(x) - x in float64, every scalar on the device (gfx950): the float64 fixed point h* at any size.
//
// replaces: broyden(f, x0, threshold, eps, stop_mode="rel", ls=False) run in double precision
//           (dirichlet/psignn/utilities/solver.py:116-207 with matvec / rmatvec :96-114), as oracle/make_golden.py runs it for the
//           stored fp64_result arrays.
//
// The host driver is one loop over an operator (b64_loop): f for the fixed point (psignn_broyden64_solve), y -> J_f(h*)^T y + grad
// for the adjoint system of the implicit backward from y = 0 (psignn_broyden64_solve_adjoint; dirichlet/psignn/model.py:210-223
// in double precision; the product is psignn_f64_vjp with add = grad, fgnn_f64_deriv.hip).
//
// The recurrences are the reference's, statement by statement (k = nstep - 1 stored pairs when step nstep is taken):
//   x_new = x + update, dx = x_new - x, g_new = f(x_new) - x_new, dg = g_new - g
//   abs = |g_new|, rel = abs / (|g_new + x_new| + 1e-9); the lowest-rel iterate is kept
//   stop: rel < eps | nstep > 30 and rel < 3 eps and max / min of the last 30 rel < 1.3 | rel > rel_0 * (1e3 * d)
//   vT = -dx + sum_j (dx . U_j) V_j              u = (dx - (-dg + sum_j (V_j . dg) U_j)) / (vT . dg)        NaN -> 0 in both
//   V_k = vT, U_k = u, update = -(-g_new + sum_{j <= k} (V_j . g_new) U_j)
// Storage: the pairs in float64, U and V (threshold, M) row-contiguous, M = N d: 2 * threshold * M * 8 bytes.
//
// One iteration (every kernel returns at once when the done flag is set, so what the host has queued past the last iteration
// changes nothing: no result depends on poll_every):
//   k_b64_step    x_new, dx                                                      (2 doubles per lane)
//   f             psignn_f64_eval (fgnn_f64.hip)
//   k_b64_resid   g_new, dg, block partials of |g_new|^2 and |g_new + x_new|^2
//   k_b64_test    one block: the two norms, trace entries, lowest, the stop tests
//   k_b64_keep    result <- x_new when this step is the lowest so far
//   k_b64_dots    sweep 1 over the k stored pairs: partials of a_j = dx . U_j, b_j = V_j . dg, c_j = V_j . g_new
//   k_b64_coef    one block per pair: the three sums
//   k_b64_comb    sweep 2 over the k stored pairs: vT -> V_k, w = dx - (-dg + sum b_j U_j), t = -g_new + sum c_j U_j, partials of
//                 vT . dg and V_k . g_new
//   k_b64_den     one block: those two sums
//   k_b64_apply   u = w / (vT . dg) -> U_k, update = -(t + (V_k . g_new) u)
// The two sweeps are the two-pass form: each reads the 2 k M stored doubles once, 16 bytes per lane, consecutive lanes consecutive
// addresses.  Sweep 1 gives a wave one pair at a time over a chunk of 1024 elements whose dx, dg, g_new sit in LDS, so one wave
// reduction serves 16 KiB of streamed history; sweep 2 gives a lane two elements and walks the pairs in ascending order.
// Reductions (f64_common.h): per-wave / per-block partials, then one block sums the partials, all in a fixed order: the same call
// gives the same bits.
#include "f64_common.h"
#include <math.h>

struct B64State {
  double lowest, lowest_abs, den, ck;
  int32_t nstep, done, low_step, low_step_abs, prot_break, stop_reason, improved_at, pad_;
};

struct psignn_broyden64 {
  psignn_f64_t* f = nullptr;   // borrowed
  int64_t N = 0, M = 0, nblk = 0, nchunk = 0;
  int threshold = 0;
  double *U = nullptr, *V = nullptr;   // (threshold, M) each
  double* vec = nullptr;               // 10 vectors of M: x0 x1 g0 g1 fx dx dg upd w t
  double* part = nullptr;              // 2 planes of nblk block partials
  double* partA = nullptr;             // (threshold, 3, nchunk) sweep-1 partials
  double* coef = nullptr;              // (threshold, 3) a_j b_j c_j
  double *rel_trace = nullptr, *abs_trace = nullptr;   // (threshold) device
  B64State* st = nullptr;              // device
  B64State* h_st = nullptr;            // pinned
};

__device__ __forceinline__ double b64_nan0(double v) { return v != v ? 0.0 : v; }

// ------------------------------------------------------------------ start
__global__ void k_b64_init(B64State* st) {
  B64State s{};
  s.lowest = 1e8;
  s.lowest_abs = 1e8;
  *st = s;
}
// x <- x0, result <- x0 (the reference's lowest_xest before any step)
__global__ void k_b64_load(int64_t M, const double* __restrict__ x0, double* __restrict__ x, double* __restrict__ result) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M) return;
  const double v = x0[i];
  x[i] = v;
  result[i] = v;
}
// g = f(x0) - x0, update = -matvec(no pairs, g) = -(-g)
__global__ void k_b64_begin(int64_t M, const double* __restrict__ fx, const double* __restrict__ x, double* __restrict__ g,
                            double* __restrict__ upd) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M) return;
  const double gi = fx[i] - x[i];
  g[i] = gi;
  upd[i] = -(-gi);
}

// ------------------------------------------------------------------ one iteration
__global__ void __launch_bounds__(F64_TB) k_b64_step(int64_t M, const B64State* __restrict__ st, const double* __restrict__ xo,
                                                     const double* __restrict__ upd, double* __restrict__ xn, double* __restrict__ dx) {
  if (st->done) return;
  const int64_t e = ((int64_t)blockIdx.x * F64_TB + threadIdx.x) * 2;
  if (e >= M) return;   // M is even: a lane's two elements are both inside or both outside
  const double2 a = *(const double2*)(xo + e), u = *(const double2*)(upd + e);
  double2 n, d;
  n.x = a.x + u.x;
  n.y = a.y + u.y;
  d.x = n.x - a.x;
  d.y = n.y - a.y;
  *(double2*)(xn + e) = n;
  *(double2*)(dx + e) = d;
}

__global__ void __launch_bounds__(F64_TB) k_b64_resid(int64_t M, int64_t nblk, const B64State* __restrict__ st,
                                                      const double* __restrict__ fx, const double* __restrict__ xn,
                                                      const double* __restrict__ go, double* __restrict__ gn, double* __restrict__ dg,
                                                      double* __restrict__ part) {
  if (st->done) return;
  __shared__ double sh[4];
  const int64_t e = ((int64_t)blockIdx.x * F64_TB + threadIdx.x) * 2;
  double gg = 0.0, ss = 0.0;
  if (e < M) {
    const double2 f = *(const double2*)(fx + e), x = *(const double2*)(xn + e), o = *(const double2*)(go + e);
    double2 g, d;
    g.x = f.x - x.x;
    g.y = f.y - x.y;
    d.x = g.x - o.x;
    d.y = g.y - o.y;
    *(double2*)(gn + e) = g;
    *(double2*)(dg + e) = d;
    const double s0 = g.x + x.x, s1 = g.y + x.y;
    gg = fma(g.y, g.y, g.x * g.x);
    ss = fma(s1, s1, s0 * s0);
  }
  gg = f64_block_sum(gg, sh);
  ss = f64_block_sum(ss, sh);
  if (threadIdx.x == 0) {
    part[blockIdx.x] = gg;
    part[nblk + blockIdx.x] = ss;
  }
}

__global__ void __launch_bounds__(F64_TB) k_b64_test(B64State* st, const double* __restrict__ part, int64_t nblk, double eps,
                                                     int threshold, double* __restrict__ rel_trace, double* __restrict__ abs_trace) {
  if (st->done) return;
  __shared__ double sh[4];
  const double gg = f64_final_sum(part, nblk, sh);
  const double ss = f64_final_sum(part + nblk, nblk, sh);
  if (threadIdx.x != 0) return;
  const int32_t nstep = st->nstep + 1;
  st->nstep = nstep;
  const double abs_diff = sqrt(gg);
  const double rel_diff = abs_diff / (sqrt(ss) + 1e-9);
  abs_trace[nstep - 1] = abs_diff;
  rel_trace[nstep - 1] = rel_diff;
  if (rel_diff < st->lowest) {
    st->lowest = rel_diff;
    st->low_step = nstep;
    st->improved_at = nstep;
  }
  if (abs_diff < st->lowest_abs) {
    st->lowest_abs = abs_diff;
    st->low_step_abs = nstep;
  }
  int reason = 0;
  if (rel_diff < eps) {
    reason = 1;
  } else {
    bool plateau = false;
    if (rel_diff < 3 * eps && nstep > 30) {
      double hi = rel_trace[nstep - 30], lo = hi;
      for (int i = nstep - 29; i < nstep; ++i) {
        hi = fmax(hi, rel_trace[i]);
        lo = fmin(lo, rel_trace[i]);
      }
      plateau = hi / lo < 1.3;
    }
    if (plateau) reason = 2;
    else if (rel_diff > rel_trace[0] * (1e3 * D)) {
      reason = 3;
      st->prot_break = 1;
    }
  }
  if (reason) {
    st->stop_reason = reason;
    st->done = 1;
  } else if (nstep >= threshold) {
    st->done = 1;   // stop_reason 0: the threshold
  }
}

// NOT gated by the done flag: the step that ends the solve may be the lowest one.  `it` is the host's count of the launch; a launch
// queued past the last iteration has it > improved_at.
__global__ void k_b64_keep(int64_t M, const B64State* __restrict__ st, int it, const double* __restrict__ xn, double* __restrict__ result) {
  if (st->improved_at != it) return;
  const int64_t e = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 2;
  if (e < M) *(double2*)(result + e) = *(const double2*)(xn + e);
}

// Sweep 1.  Block = chunk of F64_CHUNK elements; its dx, dg, g_new in LDS; wave w takes pairs w, w + 4, ...  A lane reads 8 double2
// of U_j and 8 of V_j (index (i * 64 + lane) * 2 within the chunk).  partA[(j * 3 + q) * nchunk + chunk].
template <bool FULL>
__device__ __forceinline__ void b64_dots_chunk(int64_t M, int64_t nchunk, int k, const double* __restrict__ U,
                                               const double* __restrict__ V, const double* __restrict__ dx,
                                               const double* __restrict__ dg, const double* __restrict__ gn,
                                               double* __restrict__ partA, double2* s_dx, double2* s_dg, double2* s_g) {
  const int64_t base = (int64_t)blockIdx.x * F64_CHUNK;
  for (int i = threadIdx.x; i < F64_CHUNK / 2; i += F64_TB) {
    const int64_t e = base + 2 * i;
    s_dx[i] = f64_ld2<FULL>(dx, e, base, M);
    s_dg[i] = f64_ld2<FULL>(dg, e, base, M);
    s_g[i] = f64_ld2<FULL>(gn, e, base, M);
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll 1
  for (int j = wave; j < k; j += F64_TB / 64) {
    const double* Uj = U + (int64_t)j * M;
    const double* Vj = V + (int64_t)j * M;
    double2 u[8], v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int64_t e = base + (int64_t)(i * 64 + lane) * 2;
      u[i] = f64_ld2<FULL>(Uj, e, base, M);
      v[i] = f64_ld2<FULL>(Vj, e, base, M);
    }
    double a = 0.0, b = 0.0, c = 0.0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const double2 x = s_dx[i * 64 + lane], d = s_dg[i * 64 + lane], g = s_g[i * 64 + lane];
      a = fma(x.x, u[i].x, a);
      a = fma(x.y, u[i].y, a);
      b = fma(v[i].x, d.x, b);
      b = fma(v[i].y, d.y, b);
      c = fma(v[i].x, g.x, c);
      c = fma(v[i].y, g.y, c);
    }
    a = f64_wave_sum(a);
    b = f64_wave_sum(b);
    c = f64_wave_sum(c);
    if (lane == 0) {
      double* o = partA + (int64_t)j * 3 * nchunk + blockIdx.x;
      o[0] = a;
      o[nchunk] = b;
      o[2 * nchunk] = c;
    }
  }
}
__global__ void __launch_bounds__(F64_TB) k_b64_dots(int64_t M, int64_t nchunk, int k, const B64State* __restrict__ st,
                                                     const double* __restrict__ U, const double* __restrict__ V,
                                                     const double* __restrict__ dx, const double* __restrict__ dg,
                                                     const double* __restrict__ gn, double* __restrict__ partA) {
  if (st->done) return;
  __shared__ double2 s_dx[F64_CHUNK / 2], s_dg[F64_CHUNK / 2], s_g[F64_CHUNK / 2];
  if (((int64_t)blockIdx.x + 1) * F64_CHUNK <= M) b64_dots_chunk<true>(M, nchunk, k, U, V, dx, dg, gn, partA, s_dx, s_dg, s_g);
  else b64_dots_chunk<false>(M, nchunk, k, U, V, dx, dg, gn, partA, s_dx, s_dg, s_g);
}

// one block per stored pair: a_j, b_j, c_j
__global__ void __launch_bounds__(F64_TB) k_b64_coef(int64_t nchunk, const B64State* __restrict__ st, const double* __restrict__ partA,
                                                     double* __restrict__ coef) {
  if (st->done) return;
  __shared__ double sh[4];
  const int j = blockIdx.x;
  const double* p = partA + (int64_t)j * 3 * nchunk;
  const double a = f64_final_sum(p, nchunk, sh);
  const double b = f64_final_sum(p + nchunk, nchunk, sh);
  const double c = f64_final_sum(p + 2 * nchunk, nchunk, sh);
  if (threadIdx.x == 0) {
    coef[3 * j] = a;
    coef[3 * j + 1] = b;
    coef[3 * j + 2] = c;
  }
}

// Sweep 2.  Two elements per lane, pairs in ascending order.  V[k] <- vT (NaN -> 0), w, t; partials of vT . dg (the raw vT: a NaN
// there makes u NaN, which k_b64_apply zeroes, as in the reference) and of V_k . g_new (the stored, cleaned vT).
__global__ void __launch_bounds__(F64_TB) k_b64_comb(int64_t M, int64_t nblk, int k, const B64State* __restrict__ st,
                                                     const double* __restrict__ U, double* __restrict__ V,
                                                     const double* __restrict__ coef, const double* __restrict__ dx,
                                                     const double* __restrict__ dg, const double* __restrict__ gn,
                                                     double* __restrict__ w, double* __restrict__ t, double* __restrict__ part) {
  if (st->done) return;
  __shared__ double sh[4];
  const int64_t e = ((int64_t)blockIdx.x * F64_TB + threadIdx.x) * 2;
  double den = 0.0, ck = 0.0;
  if (e < M) {
    double2 sa = {0.0, 0.0}, sb = {0.0, 0.0}, sc = {0.0, 0.0};
#pragma unroll 4
    for (int j = 0; j < k; ++j) {
      const double a = coef[3 * j], b = coef[3 * j + 1], c = coef[3 * j + 2];
      const double2 u = *(const double2*)(U + (int64_t)j * M + e), v = *(const double2*)(V + (int64_t)j * M + e);
      sa.x = fma(a, v.x, sa.x);
      sa.y = fma(a, v.y, sa.y);
      sb.x = fma(b, u.x, sb.x);
      sb.y = fma(b, u.y, sb.y);
      sc.x = fma(c, u.x, sc.x);
      sc.y = fma(c, u.y, sc.y);
    }
    const double2 x = *(const double2*)(dx + e), d = *(const double2*)(dg + e), g = *(const double2*)(gn + e);
    double2 vt, ww, tt, vc;
    vt.x = -x.x + sa.x;
    vt.y = -x.y + sa.y;
    ww.x = x.x - (-d.x + sb.x);
    ww.y = x.y - (-d.y + sb.y);
    tt.x = -g.x + sc.x;
    tt.y = -g.y + sc.y;
    vc.x = b64_nan0(vt.x);
    vc.y = b64_nan0(vt.y);
    *(double2*)(V + (int64_t)k * M + e) = vc;
    *(double2*)(w + e) = ww;
    *(double2*)(t + e) = tt;
    den = fma(vt.y, d.y, vt.x * d.x);
    ck = fma(vc.y, g.y, vc.x * g.x);
  }
  den = f64_block_sum(den, sh);
  ck = f64_block_sum(ck, sh);
  if (threadIdx.x == 0) {
    part[blockIdx.x] = den;
    part[nblk + blockIdx.x] = ck;
  }
}

__global__ void __launch_bounds__(F64_TB) k_b64_den(B64State* st, const double* __restrict__ part, int64_t nblk) {
  if (st->done) return;
  __shared__ double sh[4];
  const double den = f64_final_sum(part, nblk, sh);
  const double ck = f64_final_sum(part + nblk, nblk, sh);
  if (threadIdx.x == 0) {
    st->den = den;
    st->ck = ck;
  }
}

// u = w / (vT . dg), NaN -> 0, -> U_k; update = -(t + c_k u): the new pair's term is the last of the sum, as in the stored order
__global__ void __launch_bounds__(F64_TB) k_b64_apply(int64_t M, int k, const B64State* __restrict__ st, const double* __restrict__ w,
                                                      const double* __restrict__ t, double* __restrict__ U, double* __restrict__ upd) {
  if (st->done) return;
  const int64_t e = ((int64_t)blockIdx.x * F64_TB + threadIdx.x) * 2;
  if (e >= M) return;
  const double den = st->den, ck = st->ck;
  const double2 ww = *(const double2*)(w + e), tt = *(const double2*)(t + e);
  double2 u, up;
  u.x = b64_nan0(ww.x / den);
  u.y = b64_nan0(ww.y / den);
  up.x = -fma(ck, u.x, tt.x);
  up.y = -fma(ck, u.y, tt.y);
  *(double2*)(U + (int64_t)k * M + e) = u;
  *(double2*)(upd + e) = up;
}

// ------------------------------------------------------------------ host
extern "C" void psignn_broyden64_destroy(psignn_broyden64_t* s) {
  if (!s) return;
  void* ptrs[] = {s->U, s->V, s->vec, s->part, s->partA, s->coef, s->rel_trace, s->abs_trace, s->st};
  for (void* q : ptrs)
    if (q) (void)hipFree(q);
  if (s->h_st) (void)hipHostFree(s->h_st);
  delete s;
}

extern "C" int psignn_broyden64_create(psignn_broyden64_t** out, psignn_f64_t* f, int threshold) {
  ARG_CHECK(out != nullptr, "out is NULL");
  *out = nullptr;
  ARG_CHECK(f != nullptr, "the float64 map handle is NULL");
  ARG_CHECK(threshold >= 1 && threshold <= (1 << 20), "threshold out of range");
  const psignn_plan* p = psignn_f64_plan(f);
  ARG_CHECK(p->N > 0, "the plan has no nodes");
  psignn_broyden64* s = new psignn_broyden64();
  s->f = f;
  s->N = p->N;
  s->M = p->N * D;
  s->threshold = threshold;
  s->nblk = cdiv(s->M, 2 * F64_TB);
  s->nchunk = cdiv(s->M, F64_CHUNK);
  const size_t pair_bytes = (size_t)2 * threshold * (size_t)s->M * sizeof(double);
  double *dU = nullptr, *dV = nullptr;
  const bool got = hipMalloc((void**)&dU, pair_bytes / 2) == hipSuccess && hipMalloc((void**)&dV, pair_bytes / 2) == hipSuccess;
  s->U = got ? dU : nullptr;
  s->V = got ? dV : nullptr;
  if (!got) {
    (void)hipGetLastError();   // the failed allocation is reported here, not by the next launch
    if (dU) (void)hipFree(dU);
    psignn_set_error("psignn_broyden64_create: cannot allocate the float64 pairs: 2 * threshold * N * d * 8 = 2 * %d * %lld * %d * 8 = "
                     "%zu bytes", threshold, (long long)s->N, D, pair_bytes);
    psignn_broyden64_destroy(s);
    return PSIGNN_ENOMEM;
  }
  auto fail = [&](int code) {
    psignn_broyden64_destroy(s);
    return code;
  };
  HIP_TRY_OR(hipMalloc((void**)&s->vec, (size_t)10 * s->M * sizeof(double)), fail(PSIGNN_EHIP));
  HIP_TRY_OR(hipMalloc((void**)&s->part, (size_t)2 * s->nblk * sizeof(double)), fail(PSIGNN_EHIP));
  HIP_TRY_OR(hipMalloc((void**)&s->partA, (size_t)threshold * 3 * s->nchunk * sizeof(double)), fail(PSIGNN_EHIP));
  HIP_TRY_OR(hipMalloc((void**)&s->coef, (size_t)threshold * 3 * sizeof(double)), fail(PSIGNN_EHIP));
  HIP_TRY_OR(hipMalloc((void**)&s->rel_trace, (size_t)threshold * sizeof(double)), fail(PSIGNN_EHIP));
  HIP_TRY_OR(hipMalloc((void**)&s->abs_trace, (size_t)threshold * sizeof(double)), fail(PSIGNN_EHIP));
  HIP_TRY_OR(hipMalloc((void**)&s->st, sizeof(B64State)), fail(PSIGNN_EHIP));
  HIP_TRY_OR(hipHostMalloc((void**)&s->h_st, sizeof(B64State)), fail(PSIGNN_EHIP));
  *out = s;
  return PSIGNN_OK;
}

extern "C" size_t psignn_broyden64_bytes(const psignn_broyden64_t* s) {
  if (!s) return 0;
  return ((size_t)2 * s->threshold + 10) * (size_t)s->M * sizeof(double) +
         ((size_t)2 * s->nblk + (size_t)s->threshold * 3 * (s->nchunk + 1) + (size_t)2 * s->threshold) * sizeof(double) + sizeof(B64State);
}

// One solve of g(x) = op(x) - x.  op(x, out, done): out = the map at x on the stream, its launches returning at once when *done is
// set (NULL: no flag).  d_x0 == NULL: from x0 = 0.
template <class Op>
static int b64_loop(psignn_broyden64* s, Op&& op, const double* x0, double eps, int poll_every, double* result,
                    psignn_solve_info_t* h_info, double* h_rel_trace, double* h_abs_trace, hipStream_t st) {
  if (poll_every <= 0) poll_every = 16;
  const int64_t M = s->M, nblk = s->nblk;
  const unsigned g1 = (unsigned)cdiv(M, F64_TB), g2 = (unsigned)nblk, gc = (unsigned)s->nchunk;
  double* x[2] = {s->vec, s->vec + M};
  double* g[2] = {s->vec + 2 * M, s->vec + 3 * M};
  double *fx = s->vec + 4 * M, *dx = s->vec + 5 * M, *dg = s->vec + 6 * M, *upd = s->vec + 7 * M, *w = s->vec + 8 * M, *t = s->vec + 9 * M;
  const int32_t* done = &s->st->done;
  int rc;
  k_b64_init<<<1, 1, 0, st>>>(s->st);
  if (!x0) {   // the zero start sits in the second iterate buffer, which step 1 overwrites
    HIP_TRY(hipMemsetAsync(x[1], 0, (size_t)M * sizeof(double), st));
    x0 = x[1];
  }
  k_b64_load<<<g1, F64_TB, 0, st>>>(M, x0, x[0], result);
  if ((rc = op(x[0], fx, nullptr))) return rc;
  k_b64_begin<<<g1, F64_TB, 0, st>>>(M, fx, x[0], g[0], upd);
  for (int it = 1; it <= s->threshold; ++it) {
    const int o = (it - 1) & 1, n = it & 1, k = it - 1;
    PROF_BYTES(4 * M * 8);
    LAUNCH("k_b64_step", st, (k_b64_step<<<g2, F64_TB, 0, st>>>(M, s->st, x[o], upd, x[n], dx)));
    if ((rc = op(x[n], fx, done))) return rc;
    PROF_BYTES(5 * M * 8);
    LAUNCH("k_b64_resid", st, (k_b64_resid<<<g2, F64_TB, 0, st>>>(M, nblk, s->st, fx, x[n], g[o], g[n], dg, s->part)));
    LAUNCH("k_b64_test", st, (k_b64_test<<<1, F64_TB, 0, st>>>(s->st, s->part, nblk, eps, s->threshold, s->rel_trace, s->abs_trace)));
    k_b64_keep<<<g2, F64_TB, 0, st>>>(M, s->st, it, x[n], result);
    if (it < s->threshold) {   // the pair of the last allowed step is never used
      if (k > 0) {
        PROF_BYTES(((int64_t)2 * k + 3) * M * 8);
        LAUNCH("k_b64_dots", st, (k_b64_dots<<<gc, F64_TB, 0, st>>>(M, s->nchunk, k, s->st, s->U, s->V, dx, dg, g[n], s->partA)));
        LAUNCH("k_b64_coef", st, (k_b64_coef<<<(unsigned)k, F64_TB, 0, st>>>(s->nchunk, s->st, s->partA, s->coef)));
      }
      PROF_BYTES(((int64_t)2 * k + 6) * M * 8);
      LAUNCH("k_b64_comb", st, (k_b64_comb<<<g2, F64_TB, 0, st>>>(M, nblk, k, s->st, s->U, s->V, s->coef, dx, dg, g[n], w, t, s->part)));
      LAUNCH("k_b64_den", st, (k_b64_den<<<1, F64_TB, 0, st>>>(s->st, s->part, nblk)));
      PROF_BYTES(4 * M * 8);
      LAUNCH("k_b64_apply", st, (k_b64_apply<<<g2, F64_TB, 0, st>>>(M, k, s->st, w, t, s->U, upd)));
    }
    if (it % poll_every == 0 && it < s->threshold) {
      HIP_TRY(hipMemcpyAsync(s->h_st, s->st, sizeof(B64State), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      if (s->h_st->done) break;
    }
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(s->h_st, s->st, sizeof(B64State), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const B64State& h = *s->h_st;
  const int n_it = h.nstep;
  if (n_it < 0 || n_it > s->threshold) {
    psignn_set_error("psignn_broyden64: internal: %d iterations recorded, threshold %d", n_it, s->threshold);
    return PSIGNN_EHIP;
  }
  if (h_rel_trace && n_it > 0) HIP_TRY(hipMemcpy(h_rel_trace, s->rel_trace, (size_t)n_it * sizeof(double), hipMemcpyDeviceToHost));
  if (h_abs_trace && n_it > 0) HIP_TRY(hipMemcpy(h_abs_trace, s->abs_trace, (size_t)n_it * sizeof(double), hipMemcpyDeviceToHost));
  h_info->nstep = h.low_step;
  h_info->n_iter = n_it;
  h_info->prot_break = h.prot_break;
  h_info->stop_reason = h.stop_reason;
  h_info->lowest = h.lowest;
  h_info->lowest_abs = h.lowest_abs;
  return PSIGNN_OK;
}

extern "C" int psignn_broyden64_solve(psignn_broyden64_t* s, const double* W, int nl, const double* x0, const double* h0,
                                      const double* prb, const double* nrm, double eps, int poll_every, double* result,
                                      psignn_solve_info_t* h_info, double* h_rel_trace, double* h_abs_trace, void* stream) {
  ARG_CHECK(s && W && x0 && h0 && prb && result && h_info, "NULL argument");
  ARG_CHECK(eps >= 0.0 && eps < INFINITY, "eps must be finite and >= 0");
  hipStream_t st = (hipStream_t)stream;
  auto f = [&](const double* x, double* out, const int32_t* done) { return psignn_f64_eval(s->f, W, nl, x, h0, prb, nrm, out, done, st); };
  return b64_loop(s, f, x0, eps, poll_every, result, h_info, h_rel_trace, h_abs_trace, st);
}

// The adjoint system of the implicit backward with the same recurrences: the map is y -> J_f(h*)^T y + grad, one psignn_f64_vjp with
// add = grad per step (what the reference's hook hands to broyden, dirichlet/psignn/model.py:210-223), from y = 0.
extern "C" int psignn_broyden64_solve_adjoint(psignn_broyden64_t* s, const double* W, int nl, const double* h_star, const double* h0,
                                              const double* prb, const double* nrm, const double* grad, double eps, int poll_every,
                                              double* work, int64_t work_doubles, double* result, psignn_solve_info_t* h_info,
                                              double* h_rel_trace, double* h_abs_trace, void* stream) {
  ARG_CHECK(s && W && h_star && h0 && prb && grad && work && result && h_info, "NULL argument");
  ARG_CHECK(eps >= 0.0 && eps < INFINITY, "eps must be finite and >= 0");
  hipStream_t st = (hipStream_t)stream;
  auto f = [&](const double* y, double* out, const int32_t* done) {
    return psignn_f64_vjp_gated(s->f, W, nl, h_star, h0, prb, nrm, y, grad, out, work, work_doubles, done, st);
  };
  return b64_loop(s, f, nullptr, eps, poll_every, result, h_info, h_rel_trace, h_abs_trace, st);
}
