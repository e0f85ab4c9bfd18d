// The small dense part of GMRES in float64, host and device: the Hessenberg least-squares problem by Givens rotations.
//
// replaces: nothing executable in the reference (its backward hook, dirichlet/psignn/model.py:210-223, solves the adjoint system
//           with Broyden); the statements are those of gmres_adjoint in tests/adjoint_gmres_ref.py, one to one.
//
// R is column-major with leading dimension ld >= k + 1: column j holds the j + 1 entries of the rotated column (upper triangle).
// Includes nothing from the project: tests/host/gmres_dense_check.cpp compiles it with a host compiler and checks it against a
// least-squares solve of random Hessenberg matrices.
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GMD_HD __host__ __device__
#else
#define GMD_HD
#endif

// Column j of the Hessenberg matrix, col[0 .. j + 1] (the shift already on col[j], the new vector's norm in col[j + 1]): apply the
// j earlier rotations, form rotation j (cs[j], sn[j]; (1, 0) for a zero pair), leave the rotated column in col (col[j] = r,
// col[j + 1] = 0) and update g[j], g[j + 1].  Returns |g[j + 1]|, the residual of the least-squares problem after j + 1 columns.
GMD_HD inline double gmd_column(int j, double* col, double* cs, double* sn, double* g) {
  for (int i = 0; i < j; ++i) {
    const double t = cs[i] * col[i] + sn[i] * col[i + 1];
    col[i + 1] = -sn[i] * col[i] + cs[i] * col[i + 1];
    col[i] = t;
  }
  const double a = col[j], b = col[j + 1];
  const double r = hypot(a, b);
  const double c = r > 0.0 ? a / r : 1.0, s = r > 0.0 ? b / r : 0.0;
  cs[j] = c;
  sn[j] = s;
  col[j] = r;
  col[j + 1] = 0.0;
  g[j + 1] = -s * g[j];
  g[j] = c * g[j];
  return fabs(g[j + 1]);
}

// ---- augmented restarts (LGMRES): the plan of a cycle and the ring of kept corrections, integers only.
// tests/host/lgmres_plan_check.cpp compiles these with a host compiler and checks them over every small case.
//
// The plan: of the `left` steps a cycle may take, the last ka search the newest kept corrections, the first nk = left - ka are
// Krylov steps; at least one Krylov step always runs.  `stored`: corrections in the ring; `augment`: how many the solve keeps.
GMD_HD inline int lgm_plan_ka(int stored, int augment, int left) {
  int ka = stored < augment ? stored : augment;
  if (ka > left - 1) ka = left - 1;
  return ka > 0 ? ka : 0;
}
GMD_HD inline int lgm_plan_nk(int stored, int augment, int left) { return left - lgm_plan_ka(stored, augment, left); }
// The ring has nslots = (the handle's augment) + 1 slots and a head, the slot that is due: the next correction is written there,
// which is never one of the <= nslots - 1 newest, so a cycle's combine may write it while it reads them.
GMD_HD inline int lgm_slot_due(int head) { return head; }
GMD_HD inline int lgm_slot_newest(int head, int nslots, int i /* 0: the newest; i < nslots - 1 */) {
  int s = head - 1 - i;
  return s < 0 ? s + nslots : s;
}
GMD_HD inline int lgm_push(int head, int nslots) { return head + 1 == nslots ? 0 : head + 1; }
GMD_HD inline int lgm_stored_after_push(int stored, int augment) { return stored < augment ? stored + 1 : augment; }

// z = R^{-1} g for the first k columns; a zero pivot gives z_i = 0.
GMD_HD inline void gmd_backsolve(int k, int ld, const double* R, const double* g, double* z) {
  for (int i = k - 1; i >= 0; --i) {
    double s = g[i];
    for (int q = i + 1; q < k; ++q) s -= R[(long long)q * ld + i] * z[q];
    const double d = R[(long long)i * ld + i];
    z[i] = d != 0.0 ? s / d : 0.0;
  }
}
