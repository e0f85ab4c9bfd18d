// Newton-Krylov in float64 for the fixed point of f, g(x) = f(x) - x = 0, with a pseudo-transient shift, every vector and norm on the
// device (gfx950): a second float64 solver beside psignn_broyden64_solve, for the sizes at which Broyden stalls (I - J_f is
// indefinite there: Ritz values of J_f reach 1.15, and (1 + sigma) I - J_f with sigma > 0.15 is not).
//
// replaces: solver(f, x0, threshold, eps) of DeepEquilibrium.forward run in double precision (dirichlet/psignn/model.py:184-207,
//           the reference's --precision switch); the reference has Broyden and Anderson there, no Newton method.
//
// Attempted step n, all on the stream:
//   psignn_gmres64_solve_shifted   (1 + sigma_n) delta = J_f(x_n) delta + g(x_n) from delta = 0, to |r| <= eta |g| (krylov_f64.hip)
//   k_nt64_add      x_t = x_n + delta
//   psignn_f64_eval f(x_t)
//   k_nt64_resid    g_t = f(x_t) - x_t (over delta, which is spent), block partials of |g_t|^2 and |f(x_t)|^2
//   k_nt64_norms    one block: both sums in a fixed order, the two norms
// (the three kernels: krylov_f64.hip, beside the vector kernels of the linear solve; this unit is host code)
// The host reads the two norms and decides (psignn_newton64_policy, host only): a rejected step leaves x, f(x) and g as they were,
// bit for bit, and raises sigma; an accepted one swaps the trial vectors in and lowers sigma with |g| (switched evolution
// relaxation), to exactly 0 below sigma_off -- plain inexact Newton from there on.  The lowest-rel accepted state is kept in
// d_result.  rel = |g| / (|f(x)| + 1e-9): Broyden's measure, stop mode "rel".
// The decision depends on the norms alone, the norms on fixed-order sums: the same call gives the same bits, whatever poll_every.
#include "internal.h"
#include <math.h>
#include <utility>

struct psignn_newton64 {
  psignn_f64_t* f = nullptr;        // borrowed
  psignn_gmres64_t* gm = nullptr;   // owned: the linear solver, restart length m
  int64_t N = 0, M = 0, nblk = 0;
  int m = 0;
  double* vec = nullptr;     // ws::newton64_vecs: x, f(x), g, x_t, f(x_t), delta
  double* part = nullptr;    // 2 planes of nblk block partials
  double* norms = nullptr;   // device: |g|, |f|
  double* h_norms = nullptr;   // pinned
};

// ------------------------------------------------------------------ the policy (host only: no device is touched)
extern "C" double psignn_newton64_policy(double sigma, double g_old, double g_new, double growth, double reject_floor,
                                         double sigma_off, int* accept) {
  if (!isfinite(g_new) || g_new > growth * g_old) {
    if (accept) *accept = 0;
    const double up = 4.0 * sigma;
    return up > reject_floor ? up : reject_floor;
  }
  if (accept) *accept = 1;
  const double next = sigma * g_new / g_old;   // switched evolution relaxation
  return next >= sigma_off ? next : 0.0;       // (a NaN, from 0 / 0, is 0 too)
}

// ------------------------------------------------------------------ host
extern "C" void psignn_newton64_destroy(psignn_newton64_t* s) {
  if (!s) return;
  if (s->gm) psignn_gmres64_destroy(s->gm);
  void* ptrs[] = {s->vec, s->part, s->norms};
  for (void* q : ptrs)
    if (q) (void)hipFree(q);
  if (s->h_norms) (void)hipHostFree(s->h_norms);
  delete s;
}

static int nt64_create(const char* who, psignn_newton64_t** out, psignn_f64_t* f, int m, int augment) {
  ARG_CHECK_AS(who, out != nullptr, "out is NULL");
  *out = nullptr;
  ARG_CHECK_AS(who, f != nullptr, "the float64 map handle is NULL");
  ARG_CHECK_AS(who, m >= 1 && m <= 4096, "restart length out of range (1 .. 4096)");
  const psignn_plan* p = psignn_f64_plan(f);
  ARG_CHECK_AS(who, p->N > 0, "the plan has no nodes");
  psignn_newton64* s = new psignn_newton64();
  s->f = f;
  s->N = p->N;
  s->M = p->N * D;
  s->m = m;
  s->nblk = psignn_nt64_blocks(s->M);
  auto fail = [&](int code) {
    psignn_newton64_destroy(s);
    return code;
  };
  int rc;
  // (names the basis' or the ring's bytes when they do not fit, and refuses an augment out of range)
  if ((rc = augment ? psignn_gmres64_create_aug(&s->gm, f, m, augment) : psignn_gmres64_create(&s->gm, f, m))) return fail(rc);
  const size_t vec_bytes = (size_t)ws::newton64_vecs(s->N, nullptr).total * sizeof(double);
  if (hipMalloc((void**)&s->vec, vec_bytes) != hipSuccess) {
    (void)hipGetLastError();   // the failed allocation is reported here, not by the next launch
    s->vec = nullptr;
    psignn_set_error("%s: cannot allocate the float64 state vectors: 6 * N * d * 8 = 6 * %lld * %d * 8 = %zu bytes", who,
                     (long long)s->N, D, vec_bytes);
    return fail(PSIGNN_ENOMEM);
  }
  HIP_TRY_OR(hipMalloc((void**)&s->part, (size_t)2 * s->nblk * sizeof(double)), fail(PSIGNN_EHIP));
  HIP_TRY_OR(hipMalloc((void**)&s->norms, 2 * sizeof(double)), fail(PSIGNN_EHIP));
  HIP_TRY_OR(hipHostMalloc((void**)&s->h_norms, 2 * sizeof(double)), fail(PSIGNN_EHIP));
  *out = s;
  return PSIGNN_OK;
}
extern "C" int psignn_newton64_create(psignn_newton64_t** out, psignn_f64_t* f, int m) { return nt64_create(__func__, out, f, m, 0); }
extern "C" int psignn_newton64_create_aug(psignn_newton64_t** out, psignn_f64_t* f, int m, int augment) {
  ARG_CHECK(augment >= 0, "augment out of range (0 .. min(m - 1, 8))");
  return nt64_create(__func__, out, f, m, augment);
}

extern "C" size_t psignn_newton64_bytes(const psignn_newton64_t* s) {
  if (!s) return 0;
  return psignn_gmres64_bytes(s->gm) + ((size_t)6 * s->M + (size_t)2 * s->nblk + 2) * sizeof(double);
}

// lo: the options of every linear solve ({0, 0.5}: the solves of psignn_newton64_solve)
static int nt64_solve(const char* who, psignn_newton64_t* s, const double* W, int nl, const double* x0, const double* h0,
                      const double* prb, const double* nrm, const psignn_newton64_opts_t* o, const psignn_gmres64_opts_t* lo,
                      double* work, int64_t work_doubles, double* result, psignn_newton64_info_t* h_info, double* h_rel_trace,
                      double* h_abs_trace, double* h_sigma_trace, double* h_trial_abs, int32_t* h_accepted, int32_t* h_krylov,
                      int32_t* h_lin_stop, void* stream) {
  ARG_CHECK_AS(who, s && W && x0 && h0 && prb && o && lo && result && h_info, "NULL argument");
  ARG_CHECK_AS(who, lo->augment >= 0 && lo->augment <= psignn_gmres64_augment(s->gm), "augment out of range (0 .. the handle's augment)");
  ARG_CHECK_AS(who, lo->stall > 0.0 && lo->stall <= 1.0, "stall must be in (0, 1]");   // (a NaN is not)
  ARG_CHECK_AS(who, nl >= 1 && nl <= 64, "n_layers out of range");
  ARG_CHECK_AS(who, o->eps >= 0.0 && o->eps < INFINITY, "eps must be finite and >= 0");
  ARG_CHECK_AS(who, o->eta >= 0.0 && o->eta < INFINITY, "eta must be finite and >= 0");
  ARG_CHECK_AS(who, o->sigma0 >= 0.0 && o->sigma0 < INFINITY, "sigma0 must be finite and >= 0");
  ARG_CHECK_AS(who, o->growth > 0.0 && o->growth < INFINITY, "growth must be finite and > 0");
  ARG_CHECK_AS(who, o->reject_floor > 0.0 && o->reject_floor < INFINITY, "reject_floor must be finite and > 0");
  ARG_CHECK_AS(who, o->sigma_off >= 0.0 && o->sigma_off < INFINITY, "sigma_off must be finite and >= 0");
  ARG_CHECK_AS(who, o->threshold >= 1 && o->threshold <= (1 << 20), "threshold out of range");
  ARG_CHECK_AS(who, o->max_rejects >= 1, "max_rejects must be >= 1");
  ARG_CHECK_AS(who, o->max_products >= 1 && o->max_products <= (1 << 24), "max_products out of range");
  ARG_CHECK_AS(who, result != x0, "result must not alias x0");
  hipStream_t st = (hipStream_t)stream;
  const int64_t M = s->M;
  const size_t vbytes = (size_t)M * sizeof(double);
  const ws::Newton64Vecs v = ws::newton64_vecs(s->N, s->vec);
  double *x = v.x, *fx = v.fx, *g = v.g, *xt = v.xt, *fxt = v.fxt, *delta = v.delta;
  int rc;
  // |g| and |f| at (x, fx), g written to gout; one host read
  auto norms = [&](const double* xx, const double* ff, double* gout, double* ng, double* nf) -> int {
    psignn_nt64_resid_norms(M, ff, xx, gout, s->part, s->norms, st);
    HIP_TRY(hipMemcpyAsync(s->h_norms, s->norms, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *ng = s->h_norms[0];
    *nf = s->h_norms[1];
    return PSIGNN_OK;
  };
  HIP_TRY(hipMemcpyAsync(x, x0, vbytes, hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipMemcpyAsync(result, x0, vbytes, hipMemcpyDeviceToDevice, st));
  if ((rc = psignn_f64_eval(s->f, W, nl, x, h0, prb, nrm, fx, nullptr, st))) return rc;
  double ng, nf;
  if ((rc = norms(x, fx, g, &ng, &nf))) return rc;
  double rel = ng / (nf + 1e-9), lowest = rel, lowest_abs = ng, sigma = o->sigma0;
  int n_acc = 0, low_step = 0, products = 0, fevals = 1, rejects = 0, n = 0, stop = PSIGNN_NEWTON_THRESHOLD;
  if (h_rel_trace) h_rel_trace[0] = rel;
  if (h_abs_trace) h_abs_trace[0] = ng;
  if (h_sigma_trace) h_sigma_trace[0] = sigma;
  while (true) {
    if (rel < o->eps) {
      stop = PSIGNN_NEWTON_TOLERANCE;
      break;
    }
    if (rejects >= o->max_rejects) {
      stop = PSIGNN_NEWTON_REJECTS;
      break;
    }
    if (n >= o->threshold) break;
    psignn_gmres64_info_t lin;
    if ((rc = psignn_gmres64_solve_shifted_opts(s->gm, W, nl, x, h0, prb, nrm, g, 1.0 + sigma, 0, o->eta, o->max_products, o->poll_every,
                                                lo, work, work_doubles, delta, &lin, nullptr, nullptr, stream)))
      return rc;
    psignn_nt64_add(M, x, delta, xt, st);
    if ((rc = psignn_f64_eval(s->f, W, nl, xt, h0, prb, nrm, fxt, nullptr, st))) return rc;
    double ngt, nft;
    if ((rc = norms(xt, fxt, delta, &ngt, &nft))) return rc;   // g_t over delta: x_t holds the step already
    ++fevals;
    products += lin.products;
    int accept = 0;
    sigma = psignn_newton64_policy(sigma, ng, ngt, o->growth, o->reject_floor, o->sigma_off, &accept);
    if (h_trial_abs) h_trial_abs[n] = ngt;
    if (h_accepted) h_accepted[n] = accept;
    if (h_krylov) h_krylov[n] = lin.products;
    if (h_lin_stop) h_lin_stop[n] = lin.stop_reason;
    if (h_sigma_trace) h_sigma_trace[n + 1] = sigma;
    ++n;
    if (!accept) {
      ++rejects;
      continue;
    }
    rejects = 0;
    std::swap(x, xt);
    std::swap(fx, fxt);
    std::swap(g, delta);
    ng = ngt;
    nf = nft;
    rel = ng / (nf + 1e-9);
    ++n_acc;
    if (h_rel_trace) h_rel_trace[n_acc] = rel;
    if (h_abs_trace) h_abs_trace[n_acc] = ng;
    if (rel < lowest) {
      lowest = rel;
      lowest_abs = ng;
      low_step = n_acc;
      HIP_TRY(hipMemcpyAsync(result, x, vbytes, hipMemcpyDeviceToDevice, st));
    }
  }
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipGetLastError());
  h_info->nstep = low_step;
  h_info->n_iter = n;
  h_info->n_accepted = n_acc;
  h_info->n_products = products;
  h_info->n_feval = fevals;
  h_info->stop_reason = stop;
  h_info->lowest = lowest;
  h_info->lowest_abs = lowest_abs;
  return PSIGNN_OK;
}
extern "C" int psignn_newton64_solve(psignn_newton64_t* s, const double* W, int nl, const double* x0, const double* h0,
                                     const double* prb, const double* nrm, const psignn_newton64_opts_t* o, double* work,
                                     int64_t work_doubles, double* result, psignn_newton64_info_t* h_info, double* h_rel_trace,
                                     double* h_abs_trace, double* h_sigma_trace, double* h_trial_abs, int32_t* h_accepted,
                                     int32_t* h_krylov, int32_t* h_lin_stop, void* stream) {
  const psignn_gmres64_opts_t plain = {0, 0.5};
  return nt64_solve(__func__, s, W, nl, x0, h0, prb, nrm, o, &plain, work, work_doubles, result, h_info, h_rel_trace, h_abs_trace,
                    h_sigma_trace, h_trial_abs, h_accepted, h_krylov, h_lin_stop, stream);
}
extern "C" int psignn_newton64_solve_opts(psignn_newton64_t* s, const double* W, int nl, const double* x0, const double* h0,
                                          const double* prb, const double* nrm, const psignn_newton64_opts_t* o,
                                          const psignn_gmres64_opts_t* lo, double* work, int64_t work_doubles, double* result,
                                          psignn_newton64_info_t* h_info, double* h_rel_trace, double* h_abs_trace,
                                          double* h_sigma_trace, double* h_trial_abs, int32_t* h_accepted, int32_t* h_krylov,
                                          int32_t* h_lin_stop, void* stream) {
  return nt64_solve(__func__, s, W, nl, x0, h0, prb, nrm, o, lo, work, work_doubles, result, h_info, h_rel_trace, h_abs_trace,
                    h_sigma_trace, h_trial_abs, h_accepted, h_krylov, h_lin_stop, stream);
}
