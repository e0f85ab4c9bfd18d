// Host check of csrc/gmres_dense.h (the only project header included): random (k + 1, k) Hessenberg matrices H, right-hand side
// beta e_1.  The columns go through gmd_column one at a time as the Arnoldi loop feeds them, then gmd_backsolve; the result is
// compared with an independent least-squares solve (Householder QR in long double), the residual norm it reports with |b - H z|,
// and H^T (b - H z) with zero.  Also: a zero column pair (rotation (1, 0)), a zero pivot (z_i = 0), k = 1.
// Prints one line per case and "ok"; any miss is exit code 1.
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

#include "gmres_dense.h"

using ld_t = long double;

// min |b - H z| over z by Householder QR in long double; H (rows, cols) column-major
static std::vector<double> lstsq(std::vector<ld_t> A, std::vector<ld_t> b, int rows, int cols) {
  for (int c = 0; c < cols; ++c) {
    ld_t nrm = 0;
    for (int r = c; r < rows; ++r) nrm += A[c * rows + r] * A[c * rows + r];
    nrm = std::sqrt(nrm);
    if (nrm == 0) continue;
    const ld_t alpha = A[c * rows + c] > 0 ? -nrm : nrm;
    std::vector<ld_t> v(rows, 0);
    for (int r = c; r < rows; ++r) v[r] = A[c * rows + r];
    v[c] -= alpha;
    ld_t vv = 0;
    for (int r = c; r < rows; ++r) vv += v[r] * v[r];
    if (vv == 0) continue;
    auto reflect = [&](ld_t* x) {
      ld_t d = 0;
      for (int r = c; r < rows; ++r) d += v[r] * x[r];
      d = 2 * d / vv;
      for (int r = c; r < rows; ++r) x[r] -= d * v[r];
    };
    for (int q = c; q < cols; ++q) reflect(&A[q * rows]);
    reflect(b.data());
  }
  std::vector<double> z(cols);
  std::vector<ld_t> zl(cols);
  for (int i = cols - 1; i >= 0; --i) {
    ld_t s = b[i];
    for (int q = i + 1; q < cols; ++q) s -= A[q * rows + i] * zl[q];
    zl[i] = s / A[i * rows + i];
    z[i] = (double)zl[i];
  }
  return z;
}

static int fails = 0;
#define CHECK(cond, ...)            \
  do {                              \
    if (!(cond)) {                  \
      std::printf("FAIL " __VA_ARGS__); \
      std::printf("\n");            \
      ++fails;                      \
    }                               \
  } while (0)

static void random_case(int k, unsigned seed, double diag_shift) {
  std::mt19937_64 gen(seed);
  std::normal_distribution<double> nd(0.0, 1.0);
  const int rows = k + 1, ld = k + 3;   // a leading dimension larger than the column, as the solver's (m + 1) is for short cycles
  std::vector<double> H(rows * k, 0.0);
  for (int j = 0; j < k; ++j) {
    for (int i = 0; i <= j; ++i) H[j * rows + i] = nd(gen);
    H[j * rows + j] += diag_shift;
    H[j * rows + j + 1] = std::fabs(nd(gen)) + 0.05;   // the norm of the new vector
  }
  const double beta = 1.0 + std::fabs(nd(gen));
  std::vector<double> R(ld * k, 0.0), cs(k), sn(k), g(k + 1, 0.0), col(k + 2), z(k);
  g[0] = beta;
  double resid = beta;
  for (int j = 0; j < k; ++j) {
    for (int i = 0; i <= j + 1; ++i) col[i] = H[j * rows + i];
    resid = gmd_column(j, col.data(), cs.data(), sn.data(), g.data());
    CHECK(col[j + 1] == 0.0 && col[j] >= 0.0, "k %d column %d: rotated column", k, j);
    // c and s carry the rounding of hypot (1 ulp) and of a division each: c^2 + s^2 is within about 8 x 1.1e-16 of 1
    CHECK(std::fabs(cs[j] * cs[j] + sn[j] * sn[j] - 1.0) < 2e-15, "k %d column %d: rotation not unit", k, j);
    for (int i = 0; i <= j; ++i) R[j * ld + i] = col[i];
  }
  gmd_backsolve(k, ld, R.data(), g.data(), z.data());
  std::vector<ld_t> A(H.begin(), H.end()), b(rows, 0);
  b[0] = beta;
  const std::vector<double> want = lstsq(A, b, rows, k);
  double dz = 0, nz = 0, cond_proxy = 0;
  for (int i = 0; i < k; ++i) {
    dz += (z[i] - want[i]) * (z[i] - want[i]);
    nz += want[i] * want[i];
    cond_proxy = std::fmax(cond_proxy, 1.0 / std::fabs(R[i * ld + i]));
  }
  // residual b - H z, its norm against the reported one, and the normal equations
  std::vector<ld_t> r(rows, 0);
  r[0] = beta;
  for (int j = 0; j < k; ++j)
    for (int i = 0; i <= j + 1; ++i) r[i] -= (ld_t)H[j * rows + i] * z[j];
  ld_t rn = 0, hn = 0, ne = 0;
  for (int i = 0; i < rows; ++i) rn += r[i] * r[i];
  for (int j = 0; j < k; ++j) {
    ld_t d = 0;
    for (int i = 0; i <= j + 1; ++i) {
      d += (ld_t)H[j * rows + i] * r[i];
      hn += (ld_t)H[j * rows + i] * H[j * rows + i];
    }
    ne += d * d;
  }
  const double rel_z = std::sqrt(dz / nz), rel_r = std::fabs((double)std::sqrt(rn) - resid) / beta;
  const double rel_ne = (double)(std::sqrt(ne) / (std::sqrt(hn) * beta));
  std::printf("case k %3d seed %u shift %g: |z - lstsq| / |lstsq| %.2e  | |b - H z| - |g_k| | / beta %.2e  |H^T r| / (|H| beta) %.2e  max 1/|R_ii| %.1e\n",
              k, seed, diag_shift, rel_z, rel_r, rel_ne, cond_proxy);
  // float64 rotations on a matrix whose triangular factor has pivots >= 1 / cond_proxy: k * eps * growth, with a wide margin
  const double tol = 64.0 * k * 2.3e-16 * std::fmax(1.0, cond_proxy) * std::sqrt((double)hn);
  CHECK(rel_z <= tol, "k %d seed %u: z differs from the least-squares solve: %.3e > %.3e", k, seed, rel_z, tol);
  CHECK(rel_r <= 64.0 * k * 2.3e-16, "k %d seed %u: reported residual %.17g, actual %.17Lg", k, seed, resid, std::sqrt(rn));
  CHECK(rel_ne <= tol, "k %d seed %u: normal equations %.3e", k, seed, rel_ne);
}

int main() {
  for (int k : {1, 2, 3, 7, 8, 30, 50, 100})
    for (unsigned seed = 0; seed < 3; ++seed) {
      random_case(k, seed, 0.0);
      random_case(k, 100 + seed, -1.0);   // the adjoint system's shift on the diagonal
    }
  {   // a zero pair: rotation (1, 0), g unchanged, residual |g[1]| = 0
    double col[2] = {0.0, 0.0}, cs[1], sn[1], g[2] = {3.0, 0.0};
    const double res = gmd_column(0, col, cs, sn, g);
    CHECK(cs[0] == 1.0 && sn[0] == 0.0 && g[0] == 3.0 && g[1] == 0.0 && res == 0.0, "zero pair");
    double R[2] = {0.0, 0.0}, z[1] = {7.0};
    gmd_backsolve(1, 2, R, g, z);
    CHECK(z[0] == 0.0, "zero pivot gives z = 0");
  }
  {   // 3-4-5
    double col[2] = {3.0, 4.0}, cs[1], sn[1], g[2] = {10.0, 0.0};
    const double res = gmd_column(0, col, cs, sn, g);
    CHECK(col[0] == 5.0 && std::fabs(cs[0] - 0.6) < 1e-16 && std::fabs(sn[0] - 0.8) < 1e-16, "3-4-5 rotation");
    CHECK(std::fabs(g[0] - 6.0) < 1e-15 && std::fabs(g[1] + 8.0) < 1e-15 && std::fabs(res - 8.0) < 1e-15, "3-4-5 g");
  }
  if (fails) {
    std::printf("%d check(s) failed\n", fails);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
