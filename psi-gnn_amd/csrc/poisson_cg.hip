// Reference solve of the discrete Poisson system A u = y on the device: Jacobi-preconditioned conjugate gradient, float64 (gfx950).
//
// replaces: the direct solve that defines the reference's ground truth `sol` (dirichlet/dataset/extract_data.py solve(...) / LU) and
//           this repository's host stand-in for it (data/hexmesh.py _solve: scipy spsolve), which is too slow from ~30k nodes on.
//
// The system.  The plan holds the full CSR of A (a_ptr, a_col: columns ascending within a row) and the node flags.  Rows with flag
// bit0 (Dirichlet) are fixed, x_i = y_i, and none of their entries is read.  The free rows F solve the lifted system
//   A_FF x_F = b,   b = y_F - A_FD y_D,
// symmetric positive definite for a P1 stiffness matrix (the mixed family's Neumann rows are ordinary free rows).
//
// Layout.  The free rows are stored as a 64-row sliced ELL, slot-major within a slice: entry k of row 64 s + l sits at
// (slice_off[s] + k) * 64 + l, so the 64 lanes of a wave load 64 consecutive doubles and 64 consecutive int32 per slot.  A slice is as
// deep as its longest free row; shorter rows and Dirichlet rows are padded with (value 0, column = the row itself).  Dirichlet COLUMNS
// keep their values: the search direction is 0 on Dirichlet rows, so q = A p is A_FF p_F on F, and the same rows give b and the true
// residual from the full x.  One row per lane; nothing is staged in LDS (no entry is used twice).
//
// Iteration (all vectors and scalars float64, scalars in a device struct; four dependent launches):
//   k_cg_spmv    p = z + beta p_old (recomputed per gathered column from z and p_old, so no launch of its own), q = A p, partials p.q
//   k_cg_alpha   alpha = r.z / p.q                                                            (one block)
//   k_cg_update  x += alpha p, r -= alpha q, z = r / diag, partials r.z and r.r
//   k_cg_beta    beta, stop test |r| <= tol |b|, trace entry, iteration count                 (one block)
// Every kernel returns at once when the done flag is set, so whatever the host has queued beyond the last iteration changes nothing:
// result, n_iter and trace do not depend on poll_every.  Reductions (f64_common.h): one partial per block of F64_TB = 256 rows (4
// slices of 64: wave shuffles, then the four waves), then one block sums the partials, all in a fixed order: the same call gives the
// same bits.
#include "f64_common.h"
#include <math.h>

struct CgState {
  double rz, pq, alpha, beta, rr, bb, bnorm, true_rr;
  int32_t iter, done, converged, zero_b, breakdown, pad_[3];
};

struct psignn_cg {
  int64_t N = 0, nblk = 0, n_slices = 0, ell_rows = 0;
  uint8_t* flags = nullptr;          // (N) the plan's node flags (own copy: the handle does not need the plan after create)
  int32_t* slice_off = nullptr;      // (n_slices + 1) first slot-row of each slice
  double* ell_val = nullptr;         // (ell_rows, 64)
  int32_t* ell_col = nullptr;        // (ell_rows, 64)
  double* vec = nullptr;             // 7 vectors of N: diag | y | r | z | q | p0 | p1
  double *d = nullptr, *yd = nullptr, *r = nullptr, *z = nullptr, *q = nullptr, *p0 = nullptr, *p1 = nullptr;
  double* part = nullptr;            // 3 planes of nblk block partials
  CgState* st = nullptr;             // device
  CgState* h_st = nullptr;           // pinned
  double* trace = nullptr;           // (trace_cap) relative residual per iteration, device
  int64_t trace_cap = 0;
  double sym_defect = 0.0;
};

// the direction at one node from the previous direction and z -- the ONE expression both the node's own lane and every lane that
// gathers the node as a column evaluate, so that all of them hold the same bits
__device__ __forceinline__ double cg_dir(double beta, double p_old, double z) { return fma(beta, p_old, z); }

// ------------------------------------------------------------------ create: values, layout, checks
__global__ void k_cg_gather(int64_t E, const int32_t* __restrict__ eid, const void* __restrict__ a, int is_f64,
                            double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= E) return;
  const int64_t e = eid[i];
  out[i] = is_f64 ? ((const double*)a)[e] : (double)((const float*)a)[e];   // float32 widens exactly
}

// depth[s] = longest FREE row of slice s (0 when all its rows are Dirichlet rows)
__global__ void __launch_bounds__(F64_TB) k_cg_depth(int64_t N, int64_t n_slices, const uint8_t* __restrict__ flags,
                                                     const int32_t* __restrict__ a_ptr, int32_t* __restrict__ depth) {
  const int64_t i = (int64_t)blockIdx.x * F64_TB + threadIdx.x;
  int32_t len = 0;
  if (i < N && !(flags[i] & FLAG_DIRICHLET)) len = a_ptr[i + 1] - a_ptr[i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) len = max(len, __shfl_xor(len, o, 64));
  const int64_t s = i >> 6;
  if ((threadIdx.x & 63) == 0 && s < n_slices) depth[s] = len;
}

// one thread per ELL lane (n_slices * 64 of them, the tail past N included so that every slot is defined)
__global__ void __launch_bounds__(F64_TB) k_cg_fill(int64_t N, int64_t n_slices, const uint8_t* __restrict__ flags,
                                                    const int32_t* __restrict__ a_ptr, const int32_t* __restrict__ a_col,
                                                    const double* __restrict__ csr_val, const int32_t* __restrict__ slice_off,
                                                    double* __restrict__ ell_val, int32_t* __restrict__ ell_col,
                                                    double* __restrict__ diag) {
  const int64_t i = (int64_t)blockIdx.x * F64_TB + threadIdx.x;
  const int64_t s = i >> 6;
  if (s >= n_slices) return;
  const int lane = (int)(i & 63);
  const bool free_row = i < N && !(flags[i] & FLAG_DIRICHLET);
  const int32_t base = free_row ? a_ptr[i] : 0;
  const int32_t len = free_row ? a_ptr[i + 1] - base : 0;
  const int32_t self = i < N ? (int32_t)i : 0;
  const int32_t o0 = slice_off[s], o1 = slice_off[s + 1];
  double dg = 0.0;
  // padding = (value 0, column = own row; row 0 past N): it adds 0 * p[c], exactly 0 while p is finite.  A non-finite p turns the padded
  // rows NaN as well; p.Ap is then NaN and k_cg_alpha ends the solve unconverged (its test is pq > 0).
  for (int32_t k = 0; k < o1 - o0; ++k) {
    int32_t c = self;
    double v = 0.0;
    if (k < len) {
      c = a_col[base + k];
      v = csr_val[base + k];
      if (c == self) dg += v;
    }
    const int64_t e = ((int64_t)o0 + k) * 64 + lane;
    ell_val[e] = v;
    ell_col[e] = c;
  }
  if (i < N) diag[i] = free_row ? dg : 0.0;   // 0 marks a Dirichlet row for the update kernel (a free row's diagonal is checked > 0)
}

// Symmetry and definiteness evidence of A_FF.  A position given more than once is a run of equal columns in its row (the plan keeps
// every entry, ordered by (column, edge id)), and A is the SUM of a run -- that is what k_cg_fill's diagonal and every product with the
// ELL compute -- so the evidence is taken on sums: the first entry of a run adds up its run, finds the run of the transposed position
// (j, i) by binary search in row j, adds that up and compares the two sums; the later entries of a run only get the finiteness test.
// A run of one entry sums to that entry, so a matrix without repeated positions is judged by the same arithmetic as entry by entry.
// Block partials of max |A_ij - A_ji| and max |A_ij|; bad |= 1 missing transposed position, 2 diagonal of a free row not > 0, 4 a
// value that is not finite.
__global__ void __launch_bounds__(F64_TB) k_cg_check(int64_t N, const uint8_t* __restrict__ flags, const int32_t* __restrict__ a_ptr,
                                                     const int32_t* __restrict__ a_col, const double* __restrict__ csr_val,
                                                     const double* __restrict__ diag, double* __restrict__ part_def,
                                                     double* __restrict__ part_abs, int32_t* __restrict__ bad) {
  __shared__ double sh[4];
  const int64_t i = (int64_t)blockIdx.x * F64_TB + threadIdx.x;
  double def = 0.0, amax = 0.0;
  int32_t b = 0;
  if (i < N && !(flags[i] & FLAG_DIRICHLET)) {
    if (!(diag[i] > 0.0)) b |= 2;
    const int32_t k0 = a_ptr[i], k1 = a_ptr[i + 1];
    for (int32_t k = k0; k < k1; ++k) {
      const int32_t j = a_col[k];
      double v = csr_val[k];
      if (!isfinite(v)) b |= 4;
      if (k > k0 && a_col[k - 1] == j) continue;   // a later entry of a run: summed by the run's first entry
      if (flags[j] & FLAG_DIRICHLET) continue;
      for (int32_t m = k + 1; m < k1 && a_col[m] == j; ++m) v += csr_val[m];
      amax = fmax(amax, fabs(v));
      if (j == (int32_t)i) continue;
      const int32_t j1 = a_ptr[j + 1];
      int32_t lo = a_ptr[j], hi = j1;
      while (lo < hi) {   // lower bound: the first entry of the transposed run
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (a_col[mid] < (int32_t)i) lo = mid + 1; else hi = mid;
      }
      if (lo < j1 && a_col[lo] == (int32_t)i) {
        double t = csr_val[lo];
        for (int32_t m = lo + 1; m < j1 && a_col[m] == (int32_t)i; ++m) t += csr_val[m];
        def = fmax(def, fabs(v - t));
      } else {
        b |= 1;
      }
    }
  }
  if (b) atomicOr(bad, b);
  def = f64_block_max(def, sh);
  amax = f64_block_max(amax, sh);
  if (threadIdx.x == 0) {
    part_def[blockIdx.x] = def;
    part_abs[blockIdx.x] = amax;
  }
}
__global__ void __launch_bounds__(F64_TB) k_cg_check_fin(const double* __restrict__ part_def, const double* __restrict__ part_abs,
                                                         int64_t nblk, double* __restrict__ out /* 2 */) {
  __shared__ double sh[4];
  double def = 0.0, amax = 0.0;
  for (int64_t i = threadIdx.x; i < nblk; i += F64_TB) {
    def = fmax(def, part_def[i]);
    amax = fmax(amax, part_abs[i]);
  }
  def = f64_block_max(def, sh);
  amax = f64_block_max(amax, sh);
  if (threadIdx.x == 0) {
    out[0] = def;
    out[1] = amax;
  }
}

// ------------------------------------------------------------------ solve: start
__global__ void k_cg_load(int64_t N, const void* y, int y_is_f64, const double* x0, const uint8_t* __restrict__ flags,
                          double* __restrict__ yd, double* x, double* __restrict__ p0) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const double yi = y_is_f64 ? ((const double*)y)[i] : (double)((const float*)y)[i];
  const double xi = (flags[i] & FLAG_DIRICHLET) ? yi : (x0 ? x0[i] : 0.0);   // x may be x0 itself: same index, read before written
  yd[i] = yi;
  x[i] = xi;
  p0[i] = 0.0;
}

// b = y_F - A_FD y_D, r = b - A_FF x_F, z = r / diag; partials b.b, r.r, r.z (planes 0, 1, 2)
__global__ void __launch_bounds__(F64_TB) k_cg_begin(int64_t N, int64_t nblk, const int32_t* __restrict__ slice_off,
                                                     const double* __restrict__ ell_val, const int32_t* __restrict__ ell_col,
                                                     const uint8_t* __restrict__ flags, const double* __restrict__ diag,
                                                     const double* __restrict__ yd, const double* __restrict__ x,
                                                     double* __restrict__ r, double* __restrict__ z, double* __restrict__ part) {
  __shared__ double sh[4];
  const int64_t i = (int64_t)blockIdx.x * F64_TB + threadIdx.x;
  double bb = 0.0, rr = 0.0, rz = 0.0;
  if (i < N) {
    const double di = diag[i];
    double ri = 0.0, zi = 0.0;
    if (di != 0.0) {
      const int lane = (int)(i & 63);
      const int32_t o0 = slice_off[i >> 6], o1 = slice_off[(i >> 6) + 1];
      double sd = 0.0, sf = 0.0;
      for (int32_t k = o0; k < o1; ++k) {
        const int64_t e = (int64_t)k * 64 + lane;
        const int32_t c = ell_col[e];
        const double t = ell_val[e], xc = x[c];
        if (flags[c] & FLAG_DIRICHLET) sd = fma(t, xc, sd); else sf = fma(t, xc, sf);
      }
      const double bi = yd[i] - sd;
      ri = bi - sf;
      zi = ri / di;
      bb = bi * bi;
      rr = ri * ri;
      rz = ri * zi;
    }
    r[i] = ri;
    z[i] = zi;
  }
  bb = f64_block_sum(bb, sh);
  rr = f64_block_sum(rr, sh);
  rz = f64_block_sum(rz, sh);
  if (threadIdx.x == 0) {
    part[blockIdx.x] = bb;
    part[nblk + blockIdx.x] = rr;
    part[2 * nblk + blockIdx.x] = rz;
  }
}
__global__ void __launch_bounds__(F64_TB) k_cg_begin_fin(CgState* st, const double* __restrict__ part, int64_t nblk, double tol,
                                                         int max_iter, double* __restrict__ trace) {
  __shared__ double sh[4];
  const double bb = f64_final_sum(part, nblk, sh);
  const double rr = f64_final_sum(part + nblk, nblk, sh);
  const double rz = f64_final_sum(part + 2 * nblk, nblk, sh);
  if (threadIdx.x != 0) return;
  CgState s{};
  s.bb = bb;
  s.bnorm = sqrt(bb);
  s.rr = rr;
  s.rz = rz;
  if (bb == 0.0) {   // the lifted right-hand side vanishes: x_F = 0 is the solution (k_cg_zero_free stores it)
    s.zero_b = s.converged = s.done = 1;
    s.rr = 0.0;
    trace[0] = 0.0;
  } else {
    trace[0] = sqrt(rr) / s.bnorm;
    if (sqrt(rr) <= tol * s.bnorm) s.converged = s.done = 1;
    else if (max_iter <= 0) s.done = 1;
  }
  *st = s;
}
__global__ void k_cg_zero_free(int64_t N, const CgState* __restrict__ st, const uint8_t* __restrict__ flags, double* __restrict__ x) {
  if (!st->zero_b) return;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < N && !(flags[i] & FLAG_DIRICHLET)) x[i] = 0.0;
}

// ------------------------------------------------------------------ solve: one iteration
__global__ void __launch_bounds__(F64_TB) k_cg_spmv(int64_t N, const CgState* __restrict__ st, const int32_t* __restrict__ slice_off,
                                                    const double* __restrict__ ell_val, const int32_t* __restrict__ ell_col,
                                                    const double* __restrict__ z, const double* __restrict__ p_old,
                                                    double* __restrict__ p_new, double* __restrict__ q, double* __restrict__ part) {
  if (st->done) return;
  __shared__ double sh[4];
  const double beta = st->beta;
  const int64_t i = (int64_t)blockIdx.x * F64_TB + threadIdx.x;
  double pq = 0.0;
  if (i < N) {
    const int lane = (int)(i & 63);
    const int32_t o0 = slice_off[i >> 6], o1 = slice_off[(i >> 6) + 1];
    const double pi = cg_dir(beta, p_old[i], z[i]);
    double acc = 0.0;
    for (int32_t k = o0; k < o1; ++k) {
      const int64_t e = (int64_t)k * 64 + lane;
      const int32_t c = ell_col[e];
      acc = fma(ell_val[e], cg_dir(beta, p_old[c], z[c]), acc);
    }
    p_new[i] = pi;
    q[i] = acc;
    pq = pi * acc;
  }
  pq = f64_block_sum(pq, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = pq;
}
__global__ void __launch_bounds__(F64_TB) k_cg_alpha(CgState* st, const double* __restrict__ part, int64_t nblk) {
  if (st->done) return;
  __shared__ double sh[4];
  const double pq = f64_final_sum(part, nblk, sh);
  if (threadIdx.x != 0) return;
  st->pq = pq;
  if (pq > 0.0) st->alpha = st->rz / pq;
  else st->breakdown = st->done = 1;   // p.Ap <= 0 (or NaN): not positive definite at working precision; the iterate stays as it is
}
__global__ void __launch_bounds__(F64_TB) k_cg_update(int64_t N, int64_t nblk, const CgState* __restrict__ st,
                                                      const double* __restrict__ p, const double* __restrict__ q,
                                                      const double* __restrict__ diag, double* __restrict__ x, double* __restrict__ r,
                                                      double* __restrict__ z, double* __restrict__ part) {
  if (st->done) return;
  __shared__ double sh[4];
  const double alpha = st->alpha;
  const int64_t i = (int64_t)blockIdx.x * F64_TB + threadIdx.x;
  double rz = 0.0, rr = 0.0;
  if (i < N) {
    const double di = diag[i];
    if (di != 0.0) {   // Dirichlet rows keep x = y, r = z = 0
      x[i] = fma(alpha, p[i], x[i]);
      const double ri = fma(-alpha, q[i], r[i]);
      const double zi = ri / di;
      r[i] = ri;
      z[i] = zi;
      rz = ri * zi;
      rr = ri * ri;
    }
  }
  rz = f64_block_sum(rz, sh);
  rr = f64_block_sum(rr, sh);
  if (threadIdx.x == 0) {
    part[blockIdx.x] = rz;
    part[nblk + blockIdx.x] = rr;
  }
}
__global__ void __launch_bounds__(F64_TB) k_cg_beta(CgState* st, const double* __restrict__ part, int64_t nblk, double tol, int max_iter,
                                                    double* __restrict__ trace) {
  if (st->done) return;
  __shared__ double sh[4];
  const double rz = f64_final_sum(part, nblk, sh);
  const double rr = f64_final_sum(part + nblk, nblk, sh);
  if (threadIdx.x != 0) return;
  const int32_t it = st->iter + 1;
  st->iter = it;
  st->beta = rz / st->rz;
  st->rz = rz;
  st->rr = rr;
  trace[it] = sqrt(rr) / st->bnorm;
  if (sqrt(rr) <= tol * st->bnorm) st->converged = st->done = 1;
  else if (it >= max_iter) st->done = 1;
}

// ------------------------------------------------------------------ solve: the true residual |(y - A x)_F|^2
__global__ void __launch_bounds__(F64_TB) k_cg_true_res(int64_t N, const int32_t* __restrict__ slice_off,
                                                        const double* __restrict__ ell_val, const int32_t* __restrict__ ell_col,
                                                        const double* __restrict__ diag, const double* __restrict__ yd,
                                                        const double* __restrict__ x, double* __restrict__ part) {
  __shared__ double sh[4];
  const int64_t i = (int64_t)blockIdx.x * F64_TB + threadIdx.x;
  double tt = 0.0;
  if (i < N && diag[i] != 0.0) {
    const int lane = (int)(i & 63);
    const int32_t o0 = slice_off[i >> 6], o1 = slice_off[(i >> 6) + 1];
    double acc = 0.0;
    for (int32_t k = o0; k < o1; ++k) {
      const int64_t e = (int64_t)k * 64 + lane;
      acc = fma(ell_val[e], x[ell_col[e]], acc);
    }
    const double t = yd[i] - acc;
    tt = t * t;
  }
  tt = f64_block_sum(tt, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = tt;
}
__global__ void __launch_bounds__(F64_TB) k_cg_finish(CgState* st, const double* __restrict__ part, int64_t nblk) {
  __shared__ double sh[4];
  const double tt = f64_final_sum(part, nblk, sh);
  if (threadIdx.x == 0) st->true_rr = tt;
}

// ------------------------------------------------------------------ host
extern "C" void psignn_cg_destroy(psignn_cg_t* s) {
  if (!s) return;
  void* ptrs[] = {s->flags, s->slice_off, s->ell_val, s->ell_col, s->vec, s->part, s->st, s->trace};
  for (void* q : ptrs)
    if (q) (void)hipFree(q);
  if (s->h_st) (void)hipHostFree(s->h_st);
  delete s;
}

extern "C" int psignn_cg_create(psignn_cg_t** out, const psignn_plan_t* p, const void* d_a_ij, int a_is_f64, void* stream) {
  ARG_CHECK(out != nullptr, "out is NULL");
  *out = nullptr;
  ARG_CHECK(p != nullptr && d_a_ij != nullptr, "NULL argument");
  ARG_CHECK(a_is_f64 == 0 || a_is_f64 == 1, "a_is_f64 must be 0 or 1");
  ARG_CHECK(p->E > 0 && p->a_ptr && p->a_col && p->a_eid && p->flags, "the plan holds no matrix structure");
  hipStream_t st = (hipStream_t)stream;
  const int64_t N = p->N, E = p->E;
  const int64_t n_slices = cdiv(N, 64), nblk = cdiv(N, F64_TB);
  const unsigned gn = (unsigned)nblk, gl = (unsigned)cdiv(n_slices * 64, F64_TB);
  DeviceArray<double> csr_val, chk;
  DeviceArray<int32_t> depth, bsum, bad;
  psignn_cg* s = new psignn_cg();
  s->N = N;
  s->nblk = nblk;
  s->n_slices = n_slices;
  int rc = PSIGNN_OK;
  auto fail = [&](int code) {
    psignn_cg_destroy(s);
    return code;
  };
  HIP_TRY_OR(csr_val.alloc((size_t)E), fail(PSIGNN_EHIP));
  HIP_TRY_OR(chk.alloc(2), fail(PSIGNN_EHIP));
  HIP_TRY_OR(depth.alloc((size_t)n_slices), fail(PSIGNN_EHIP));
  HIP_TRY_OR(bsum.alloc((size_t)cdiv(n_slices, 1024) + 2), fail(PSIGNN_EHIP));
  HIP_TRY_OR(bad.alloc(1), fail(PSIGNN_EHIP));
  HIP_TRY_OR(hipMalloc((void**)&s->flags, (size_t)N), fail(PSIGNN_EHIP));
  HIP_TRY_OR(hipMalloc((void**)&s->slice_off, (size_t)(n_slices + 1) * sizeof(int32_t)), fail(PSIGNN_EHIP));
  HIP_TRY_OR(hipMalloc((void**)&s->vec, (size_t)7 * N * sizeof(double)), fail(PSIGNN_EHIP));
  HIP_TRY_OR(hipMalloc((void**)&s->part, (size_t)3 * nblk * sizeof(double)), fail(PSIGNN_EHIP));
  HIP_TRY_OR(hipMalloc((void**)&s->st, sizeof(CgState)), fail(PSIGNN_EHIP));
  HIP_TRY_OR(hipHostMalloc((void**)&s->h_st, sizeof(CgState)), fail(PSIGNN_EHIP));
  s->d = s->vec;
  s->yd = s->vec + N;
  s->r = s->vec + 2 * N;
  s->z = s->vec + 3 * N;
  s->q = s->vec + 4 * N;
  s->p0 = s->vec + 5 * N;
  s->p1 = s->vec + 6 * N;
  HIP_TRY_OR(hipMemcpyAsync(s->flags, p->flags, (size_t)N, hipMemcpyDeviceToDevice, st), fail(PSIGNN_EHIP));
  HIP_TRY_OR(hipMemsetAsync(bad.get(), 0, sizeof(int32_t), st), fail(PSIGNN_EHIP));
  k_cg_gather<<<(unsigned)cdiv(E, F64_TB), F64_TB, 0, st>>>(E, p->a_eid, d_a_ij, a_is_f64, csr_val.get());
  k_cg_depth<<<gl, F64_TB, 0, st>>>(N, n_slices, s->flags, p->a_ptr, depth.get());
  if ((rc = psignn_exclusive_scan(depth.get(), n_slices, s->slice_off, bsum.get(), st)) != 0) return fail(rc);
  int32_t h_rows = 0;
  HIP_TRY_OR(hipMemcpyAsync(&h_rows, s->slice_off + n_slices, sizeof(int32_t), hipMemcpyDeviceToHost, st), fail(PSIGNN_EHIP));
  HIP_TRY_OR(hipStreamSynchronize(st), fail(PSIGNN_EHIP));
  if (h_rows < 0 || h_rows > E) {   // a slice is as deep as one of its rows, so the sum never exceeds E
    psignn_set_error("psignn_cg_create: internal: %d ELL slot-rows for %lld entries", h_rows, (long long)E);
    return fail(PSIGNN_EHIP);
  }
  s->ell_rows = h_rows;
  const size_t slots = (size_t)(h_rows > 0 ? h_rows : 1) * 64;
  HIP_TRY_OR(hipMalloc((void**)&s->ell_val, slots * sizeof(double)), fail(PSIGNN_EHIP));
  HIP_TRY_OR(hipMalloc((void**)&s->ell_col, slots * sizeof(int32_t)), fail(PSIGNN_EHIP));
  k_cg_fill<<<gl, F64_TB, 0, st>>>(N, n_slices, s->flags, p->a_ptr, p->a_col, csr_val.get(), s->slice_off, s->ell_val, s->ell_col, s->d);
  k_cg_check<<<gn, F64_TB, 0, st>>>(N, s->flags, p->a_ptr, p->a_col, csr_val.get(), s->d, s->part, s->part + nblk, bad.get());
  k_cg_check_fin<<<1, F64_TB, 0, st>>>(s->part, s->part + nblk, nblk, chk.get());
  double h_chk[2] = {0.0, 0.0};
  int32_t h_bad = 0;
  HIP_TRY_OR(hipGetLastError(), fail(PSIGNN_EHIP));
  HIP_TRY_OR(hipMemcpyAsync(h_chk, chk.get(), sizeof(h_chk), hipMemcpyDeviceToHost, st), fail(PSIGNN_EHIP));
  HIP_TRY_OR(hipMemcpyAsync(&h_bad, bad.get(), sizeof(h_bad), hipMemcpyDeviceToHost, st), fail(PSIGNN_EHIP));
  HIP_TRY_OR(hipStreamSynchronize(st), fail(PSIGNN_EHIP));
  s->sym_defect = h_chk[0];
  if (h_bad & 4) {
    psignn_set_error("psignn_cg_create: a_ij holds a value that is not finite on a free row");
    return fail(PSIGNN_EINVAL);
  }
  if (h_bad & 1) {
    psignn_set_error("psignn_cg_create: the matrix is not symmetric on its free rows: an entry (i, j) has no transposed entry (j, i)");
    return fail(PSIGNN_EINVAL);
  }
  if (!(h_chk[0] <= 1e-6 * h_chk[1])) {
    psignn_set_error("psignn_cg_create: the matrix is not symmetric on its free rows: max |a_ij - a_ji| = %.3e > 1e-6 * max |a_ij| = %.3e",
                     h_chk[0], 1e-6 * h_chk[1]);
    return fail(PSIGNN_EINVAL);
  }
  if (h_bad & 2) {
    psignn_set_error("psignn_cg_create: the matrix is not symmetric positive definite on its free rows: a free row has a zero or "
                     "negative diagonal entry");
    return fail(PSIGNN_EINVAL);
  }
  *out = s;
  return PSIGNN_OK;
}

extern "C" int psignn_cg_solve(psignn_cg_t* s, const void* d_y, int y_is_f64, const double* d_x0, double tol, int max_iter,
                               int poll_every, double* d_sol, psignn_cg_info_t* h_info, double* h_res_trace, void* stream) {
  ARG_CHECK(s && d_y && d_sol && h_info, "NULL argument");
  ARG_CHECK(y_is_f64 == 0 || y_is_f64 == 1, "y_is_f64 must be 0 or 1");
  ARG_CHECK(tol >= 0.0 && tol < INFINITY, "tol must be finite and >= 0");
  ARG_CHECK(max_iter >= 0 && max_iter < INT32_MAX, "max_iter out of range");
  if (poll_every <= 0) poll_every = 50;
  hipStream_t st = (hipStream_t)stream;
  const int64_t N = s->N, nblk = s->nblk;
  const unsigned g = (unsigned)nblk;
  if (s->trace_cap < (int64_t)max_iter + 1) {
    if (s->trace) (void)hipFree(s->trace);
    s->trace = nullptr;
    s->trace_cap = 0;
    HIP_TRY(hipMalloc((void**)&s->trace, ((size_t)max_iter + 1) * sizeof(double)));
    s->trace_cap = (int64_t)max_iter + 1;
  }
  double* x = d_sol;   // the iterate lives in the caller's result array
  k_cg_load<<<g, F64_TB, 0, st>>>(N, d_y, y_is_f64, d_x0, s->flags, s->yd, x, s->p0);
  LAUNCH("k_cg_begin", st, (k_cg_begin<<<g, F64_TB, 0, st>>>(N, nblk, s->slice_off, s->ell_val, s->ell_col, s->flags, s->d, s->yd, x,
                                                            s->r, s->z, s->part)));
  k_cg_begin_fin<<<1, F64_TB, 0, st>>>(s->st, s->part, nblk, tol, max_iter, s->trace);
  k_cg_zero_free<<<g, F64_TB, 0, st>>>(N, s->st, s->flags, x);
  // algorithmic bytes of an iteration: every ELL slot once (8 + 4), z and p_old read, p and q written; then p, q, diag, x, r read,
  // x, r, z written
  const int64_t spmv_bytes = s->ell_rows * 64 * 12 + 4 * N * 8, update_bytes = 8 * N * 8;
  for (int it = 0; it < max_iter; ++it) {
    const double* p_old = (it & 1) ? s->p1 : s->p0;
    double* p_new = (it & 1) ? s->p0 : s->p1;
    PROF_BYTES(spmv_bytes);
    LAUNCH("k_cg_spmv", st, (k_cg_spmv<<<g, F64_TB, 0, st>>>(N, s->st, s->slice_off, s->ell_val, s->ell_col, s->z, p_old, p_new, s->q,
                                                            s->part)));
    LAUNCH("k_cg_alpha", st, (k_cg_alpha<<<1, F64_TB, 0, st>>>(s->st, s->part, nblk)));
    PROF_BYTES(update_bytes);
    LAUNCH("k_cg_update", st, (k_cg_update<<<g, F64_TB, 0, st>>>(N, nblk, s->st, p_new, s->q, s->d, x, s->r, s->z, s->part)));
    LAUNCH("k_cg_beta", st, (k_cg_beta<<<1, F64_TB, 0, st>>>(s->st, s->part, nblk, tol, max_iter, s->trace)));
    if ((it + 1) % poll_every == 0 && it + 1 < max_iter) {
      HIP_TRY(hipMemcpyAsync(s->h_st, s->st, sizeof(CgState), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      if (s->h_st->done) break;
    }
  }
  LAUNCH("k_cg_true_res", st, (k_cg_true_res<<<g, F64_TB, 0, st>>>(N, s->slice_off, s->ell_val, s->ell_col, s->d, s->yd, x, s->part)));
  k_cg_finish<<<1, F64_TB, 0, st>>>(s->st, s->part, nblk);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(s->h_st, s->st, sizeof(CgState), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const CgState& h = *s->h_st;
  if (h_res_trace && h.iter >= 0 && h.iter <= max_iter)
    HIP_TRY(hipMemcpy(h_res_trace, s->trace, ((size_t)h.iter + 1) * sizeof(double), hipMemcpyDeviceToHost));
  h_info->n_iter = h.iter;
  h_info->converged = h.converged;
  h_info->b_norm = h.bnorm;
  h_info->rel = h.bnorm > 0.0 ? sqrt(h.rr) / h.bnorm : 0.0;
  h_info->true_rel = h.bnorm > 0.0 ? sqrt(h.true_rr) / h.bnorm : 0.0;
  h_info->sym_defect = s->sym_defect;
  return PSIGNN_OK;
}

// =============================================================================================
// The losses of a training step in float64, on the same matrix: the residual r = A u - y of the system above with its transpose
// A^T r, and a mean-square error with its gradient.  With f, the MLPs and their backwards (fgnn_f64.hip, fgnn_f64_deriv.hip) these
// close the chain of ModelDEQDSS._train_forward in double precision (engine.train_step64).
//
// replaces: residual_loss (dirichlet/psignn/model.py:157-167: index_add_ over edge_index with a_ij, the diagonal included) and the
//           F.mse_loss terms of ModelDEQDSS.forward (model.py:58-99), with what autograd derives from them, on float64 tensors.
//
// Unlike the solve they read the plan's full CSR / CSC directly and gather the values by edge id from the caller's float64 a_ij on
// every call (no handle, every row, Dirichlet rows included).  A truth path, bound by its gathers: one row (column) per lane,
// coalesced index loads, nothing tuned further.  No atomics; every sum runs in an order that depends on the graph or on the length
// alone, so the same call gives the same bits.
// =============================================================================================
static_assert(ws::MSE64_CHUNK == F64_CHUNK && F64_CHUNK % F64_TB == 0, "one mean-square-error partial per dots chunk");

// r_i = sum_k a_ij[a_eid[k]] u[a_col[k]] - y_i over row i of the plan's full CSR (columns ascending, equal columns by edge id):
// repeated positions are added entry after entry.  The values come from the caller's float64 a_ij; the plan's own copy is fp32.
__global__ void __launch_bounds__(F64_TB) k_residual_f64(int64_t N, const int32_t* __restrict__ a_ptr, const int32_t* __restrict__ a_col,
                                                          const int32_t* __restrict__ a_eid, const double* __restrict__ a_ij,
                                                          const double* __restrict__ u, const double* __restrict__ y,
                                                          double* __restrict__ r) {
  const int64_t i = (int64_t)blockIdx.x * F64_TB + threadIdx.x;
  if (i >= N) return;
  double s = 0.0;
  for (int32_t k = a_ptr[i]; k < a_ptr[i + 1]; ++k) s += a_ij[a_eid[k]] * u[a_col[k]];
  r[i] = s - y[i];
}

// out_c = sum over the in-edges of column c (csc order: sender ascending, equal senders by edge id) of a_ij[e] r[row(e)], then the
// diagonal entries of row c in the full CSR's order: k_residual_t (fgnn_pgrad.hip) in float64, the diagonal read through a_eid too.
__global__ void __launch_bounds__(F64_TB) k_residual_t_f64(int64_t N, const int32_t* __restrict__ csc_ptr,
                                                            const int32_t* __restrict__ csc_nbr, const int32_t* __restrict__ csc_eid,
                                                            const int32_t* __restrict__ a_ptr, const int32_t* __restrict__ a_col,
                                                            const int32_t* __restrict__ a_eid, const double* __restrict__ a_ij,
                                                            const double* __restrict__ r, double* __restrict__ out) {
  const int64_t c = (int64_t)blockIdx.x * F64_TB + threadIdx.x;
  if (c >= N) return;
  double s = 0.0;
  for (int32_t k = csc_ptr[c]; k < csc_ptr[c + 1]; ++k) s += a_ij[csc_eid[k]] * r[csc_nbr[k]];
  const double rc = r[c];
  for (int32_t k = a_ptr[c]; k < a_ptr[c + 1]; ++k)
    if (a_col[k] == (int32_t)c) s += a_ij[a_eid[k]] * rc;
  out[c] = s;
}

// Block = chunk of F64_CHUNK elements: thread t takes elements t, t + 256, ... of the chunk in ascending order (8-byte loads: the
// length may be odd), then the block sum.  part[chunk] = sum (a - b)^2; grad = 2 (a - b) / scale_n, element by element.
__global__ void __launch_bounds__(F64_TB) k_mse_f64(int64_t n, const double* __restrict__ a, const double* __restrict__ b, double scale_n,
                                                     double* __restrict__ part, double* __restrict__ grad) {
  __shared__ double sh[4];
  const int64_t base = (int64_t)blockIdx.x * F64_CHUNK;
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < F64_CHUNK / F64_TB; ++i) {
    const int64_t e = base + i * F64_TB + threadIdx.x;
    if (e < n) {
      const double d = b ? a[e] - b[e] : a[e];
      s += d * d;
      if (grad) grad[e] = (2.0 * d) / scale_n;
    }
  }
  s = f64_block_sum(s, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// one block: the partials in ascending stride order, divided once
__global__ void __launch_bounds__(F64_TB) k_mse_f64_final(const double* __restrict__ part, int64_t nchunk, double scale_n,
                                                           double* __restrict__ loss) {
  __shared__ double sh[4];
  const double s = f64_final_sum(part, nchunk, sh);
  if (threadIdx.x == 0) *loss = s / scale_n;
}

static int plan_has_matrix(const psignn_plan* p) { return p->a_ptr && p->a_col && p->a_eid && p->csc_ptr && p->csc_nbr && p->csc_eid; }

extern "C" int psignn_residual_f64(const psignn_plan_t* p, const double* d_a_ij, const double* d_u, const double* d_y, double* d_r,
                                   void* stream) {
  ARG_CHECK(p && d_a_ij && d_u && d_y && d_r, "NULL argument");
  ARG_CHECK(plan_has_matrix(p), "the plan holds no matrix structure");
  ARG_CHECK(d_r != d_u && d_r != d_y, "d_r must not alias d_u or d_y");
  if (p->N == 0) return PSIGNN_OK;
  hipStream_t st = (hipStream_t)stream;
  PROF_BYTES(p->E * (4 + 4 + 8 + 8) + p->N * (4 + 8 + 8));
  LAUNCH("k_residual_f64", st,
         (k_residual_f64<<<(unsigned)cdiv(p->N, F64_TB), F64_TB, 0, st>>>(p->N, p->a_ptr, p->a_col, p->a_eid, d_a_ij, d_u, d_y, d_r)));
  HIP_TRY(hipGetLastError());
  return PSIGNN_OK;
}

extern "C" int psignn_residual_t_f64(const psignn_plan_t* p, const double* d_a_ij, const double* d_r, double* d_out, void* stream) {
  ARG_CHECK(p && d_a_ij && d_r && d_out, "NULL argument");
  ARG_CHECK(plan_has_matrix(p), "the plan holds no matrix structure");
  ARG_CHECK(d_out != d_r, "d_out must not alias d_r");
  if (p->N == 0) return PSIGNN_OK;
  hipStream_t st = (hipStream_t)stream;
  PROF_BYTES(p->Ep * (4 + 4 + 8 + 8) + p->E * (4 + 4) + p->N * (8 + 8 + 8));
  LAUNCH("k_residual_t_f64", st,
         (k_residual_t_f64<<<(unsigned)cdiv(p->N, F64_TB), F64_TB, 0, st>>>(p->N, p->csc_ptr, p->csc_nbr, p->csc_eid, p->a_ptr, p->a_col,
                                                                            p->a_eid, d_a_ij, d_r, d_out)));
  HIP_TRY(hipGetLastError());
  return PSIGNN_OK;
}

extern "C" int psignn_mse_f64_chunk(void) { return F64_CHUNK; }

extern "C" int64_t psignn_mse_f64_workspace_doubles(int64_t n_elems) { return n_elems < 1 ? -1 : ws::mse64_total(n_elems); }

extern "C" int psignn_mse_f64(const double* d_a, const double* d_b, int64_t n_elems, double scale_n, double* d_loss, double* d_grad,
                              double* d_work, int64_t work_doubles, void* stream) {
  ARG_CHECK(d_a && d_loss, "NULL argument");
  ARG_CHECK(n_elems >= 1, "n_elems must be at least 1");
  ARG_CHECK(scale_n > 0.0, "scale_n must be positive");
  ARG_CHECK(d_grad != d_a && (!d_grad || d_grad != d_b), "d_grad must not alias d_a or d_b");
  ARG_CHECK(d_loss != d_a && d_loss != d_b && d_loss != d_grad, "d_loss must not alias d_a, d_b or d_grad");
  const int64_t need = ws::mse64_total(n_elems);
  if (!d_work || work_doubles < need) {
    psignn_set_error("%s: the workspace holds %lld doubles, %lld are needed (%lld bytes)", __func__, (long long)(d_work ? work_doubles : 0),
                     (long long)need, (long long)need * 8);
    return PSIGNN_ENOMEM;
  }
  ARG_CHECK(d_work != d_a && d_work != d_b && d_work != d_grad && d_work != d_loss, "d_work must not alias an argument");
  hipStream_t st = (hipStream_t)stream;
  PROF_BYTES(n_elems * 8 * (1 + (d_b ? 1 : 0) + (d_grad ? 1 : 0)) + need * 8);
  LAUNCH("k_mse_f64", st, (k_mse_f64<<<(unsigned)need, F64_TB, 0, st>>>(n_elems, d_a, d_b, scale_n, d_work, d_grad)));
  LAUNCH("k_mse_f64_final", st, (k_mse_f64_final<<<1, F64_TB, 0, st>>>(d_work, need, scale_n, d_loss)));
  HIP_TRY(hipGetLastError());
  return PSIGNN_OK;
}
