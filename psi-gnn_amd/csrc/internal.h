// Functions called across translation units that are not part of the C API (include/psignn_hip.h): each declared once,
// grouped by the file that defines it.
#pragma once
#include "common.h"
#include "workspace.h"

// ---- the tile structures of a plan as the leading pointer arguments of a tile kernel (the order of TileCtx, common.h),
// without and with the plan-order flags
#define PLAN_TILES(p) (p)->tile_ptr, (p)->tile_slice, (p)->halo, (p)->halo_cnt, (p)->slice_off, (p)->slice_deg, (p)->ell
#define PLAN_TILES_FLAGS(p) PLAN_TILES(p), (p)->flags_p

// ---- fgnn.hip
int psignn_f_eval_p(const psignn_plan_t* p, const float* W, int nl, const float* h, const int32_t* hsel, int64_t hstride,
                    const float* h0, const float* prb, const float* nrm, float* out, float* work, hipStream_t st);
int psignn_f_gather_layer(const psignn_plan* p, const float* W, int nl, int l, const float* h, const float* h0, const float* prb,
                          const float* v, float* out, float* work, hipStream_t st);

// ---- fgnn_layers.hip
int psignn_f_layer_view(const psignn_plan* p, const float* W, int nl, int l, float* dst, hipStream_t st);
int psignn_f_dir_acc(const psignn_plan* p, const uint8_t* flags, const float* src, float* dst, int first, hipStream_t st);
int psignn_f_add_rows(const psignn_plan* p, const float* a, const float* b, float* out, hipStream_t st);
int psignn_f_layer_states(const psignn_plan* p, const float* W, int nl, const float* h, const float* prb, float* lw, float* work,
                          hipStream_t st, bool gather);
int psignn_f_layers_vjp(const psignn_plan* p, const float* W, int nl, const float* h, const float* prb, const float* w,
                        float* out, float* work, float* lw, hipStream_t st);
int psignn_f_layers_vjp_stateless(const psignn_plan* p, const float* W, int nl, const float* h, const float* prb, const float* w,
                                  float* out, float* work, float* lw, hipStream_t st);
int psignn_f_layers_jvp_stateless(const psignn_plan* p, const float* W, int nl, const float* h, const float* prb, const float* v,
                                  float* out, float* work, float* lw, hipStream_t st);

// ---- fgnn_tile.hip
int psignn_f_tile_fused_batch(const BatchDesc* d_descs, int n_mesh, int n_slots, int max_rows, const float* W, int mixed,
                              int off_done, int off_cur, int off_nxt, int par, hipStream_t st);
int psignn_f_tile_plain_batch(const FpBatchDesc* d_descs, int n_mesh, int n_slots, int max_rows, const float* W, int mixed,
                              int off_done, int in_f, int in_row, hipStream_t st);
int psignn_f_tile_forward(const psignn_plan* p, const float* W, int nl, const float* h, const int32_t* hsel, int64_t hstride,
                          const float* h0, const float* prb, const float* nrm, float* out, float* work, hipStream_t st);
int psignn_f_tile_layer(const psignn_plan* p, const float* W, int nl, int l, const float* h, const float* h0, const float* prb,
                        float* out, hipStream_t st);
int psignn_f_tile_fused(const psignn_plan* p, const float* W, int nl, float* xbuf, int64_t M, const int32_t* st_words,
                        int off_done, int off_cur, int off_nxt, const float* upd, float* gnew, const float* h0, const float* prb,
                        const float* nrm, float* part, hipStream_t st);

// ---- fgnn_tile_jr.hip
int psignn_jr_tiled_ok(const psignn_plan* p, int nl);
int psignn_jr_tile_records(const psignn_plan* p, const float* W, const float* h, const float* prb, const float* v,
                           const float* gbar, float* out_h, float* B, float* rec, hipStream_t st);

// ---- fgnn_tile_jvp.hip
int psignn_f_tile_jvp_groups(const psignn_plan* p, const float* W, int nl, const float* h, const float* prb, const float* nrm,
                             const float* v, float* out, int groups, hipStream_t st);
int psignn_f_tile_jvp_layer(const psignn_plan* p, const float* W, int nl, int l, const float* h, const float* prb, const float* v,
                            float* out, hipStream_t st);
int psignn_f_tile_jvp(const psignn_plan* p, const float* W, int nl, const float* h, const float* prb, const float* nrm,
                      const float* v, float* out, hipStream_t st);

// ---- fgnn_tile_lin.hip
const psignn_plan* psignn_lin_plan(const psignn_lin_t* s);
int psignn_lin_batch_ok(const psignn_lin_t* s, const psignn_plan* p);
int64_t psignn_lin_vjp_bytes(const psignn_lin_t* s);
int psignn_lin_batch_fill(const psignn_lin_t* s, LinBatchDesc* d, hipStream_t st);
int psignn_lin_vjp_batch(const LinBatchDesc* d_descs, int n_mesh, int n_slots, int max_rows, const float* W, int mixed,
                         int off_done, hipStream_t st);

// ---- fgnn_tile_vjp.hip
int psignn_f_tile_vjp(const psignn_plan* p, const float* W, int nl, const float* h, const float* prb, const float* nrm,
                      const float* w, float* out, float* work, hipStream_t st);
int psignn_f_tile_vjp_rec(const psignn_plan* p, const float* W, int nl, const float* h, const float* prb, const float* nrm,
                          const float* w, float* out, float* work, float* rec, hipStream_t st);
int psignn_f_tile_vjp_layer(const psignn_plan* p, const float* W, int nl, int l, const float* h, const float* prb, const float* w,
                            float* out, float* work, float* rec, hipStream_t st);

// ---- fgnn_vjp.hip
int psignn_f_gather_vjp_layer(const psignn_plan* p, const float* W, int nl, int l, const float* h, const float* prb,
                              const float* w, float* out, float* work, hipStream_t st);
int psignn_f_gather_vjp_rec_layer(const psignn_plan* p, const float* W, int nl, int l, const float* h, const float* prb,
                                  const float* nrm, const float* w, float* out, float* work, float* rec, hipStream_t st);

// ---- gather_backward.hip
int psignn_jacreg_records(const psignn_plan* p, const float* W, const float* h, const float* prb, const float* nrm,
                          const float* v, const float* gbar, float* out_h, float* work, float* rec1, float* rec2, hipStream_t st,
                          int ln);
int psignn_dsgps_step_records(const psignn_plan* p, const float* Wf, const float* Wg, const float* h, const float* prb,
                              const float* nrm, const float* w, float* out_h, float* work, float* rec, hipStream_t st);
int psignn_dss_step_records(const psignn_plan* p, const float* Wf, float alpha, const float* h, const float* bp, const float* w,
                            float* out_h, float* work, float* rec, hipStream_t st);

// ---- fgnn_f64.hip
const psignn_plan* psignn_f64_plan(const psignn_f64_t* f);
int psignn_f64_eval(psignn_f64_t* f, const double* W, int nl, const double* h, const double* h0, const double* prb, const double* nrm,
                    double* out, const int32_t* done, hipStream_t st);

// ---- fgnn_f64_deriv.hip
// psignn_f64_jvp / psignn_f64_vjp with a solver's flag: every launch of the product returns at once when *done is set (NULL: no flag)
int psignn_f64_jvp_gated(psignn_f64_t* f, const double* W, int nl, const double* h, const double* h0, const double* prb,
                         const double* nrm, const double* v, double* out, double* work, int64_t work_doubles, const int32_t* done,
                         hipStream_t st);
int psignn_f64_vjp_gated(psignn_f64_t* f, const double* W, int nl, const double* h, const double* h0, const double* prb,
                         const double* nrm, const double* w, const double* add, double* out, double* work, int64_t work_doubles,
                         const int32_t* done, hipStream_t st);

// ---- krylov_f64.hip: the vector kernels of the float64 Newton loop (newton_f64.hip).  part: 2 * psignn_nt64_blocks(M) doubles.
int64_t psignn_nt64_blocks(int64_t M);
void psignn_nt64_resid_norms(int64_t M, const double* fx, const double* x, double* g, double* part, double* norms, hipStream_t st);
void psignn_nt64_add(int64_t M, const double* x, const double* d, double* xt, hipStream_t st);
// corrections a solve on the handle may keep (psignn_gmres64_create_aug)
int psignn_gmres64_augment(const psignn_gmres64_t* s);

// ---- plan.hip
int psignn_exclusive_scan(const int32_t* in, int64_t n, int32_t* out, int32_t* bsum, hipStream_t st);

// ---- caller order <-> plan order
// The caller-numbered inputs of an entry point, copied in plan order into the rows h, x, prb, nrm of an adapter (ws::Adapter; the
// adjoint solves fill one with rows of their own): h, x (h_initial, a tangent or a cotangent; may be NULL), prb, and the unit
// normals of a mixed plan.  A row that is not filled (x; nrm on a dirichlet plan) is NULL afterwards: a.h, a.x, a.prb, a.nrm are
// then the kernel's plan-order arguments.  The result goes back with psignn_from_plan.
static inline int psignn_to_plan(const psignn_plan* p, const float* h, const float* x, const float* prb, const float* nrm,
                                 ws::Adapter& a, hipStream_t st) {
  int rc;
  if (!x) a.x = nullptr;
  if (!p->mixed) a.nrm = nullptr;
  if ((rc = psignn_plan_permute(p, h, D, a.h, 1, st))) return rc;
  if (x && (rc = psignn_plan_permute(p, x, D, a.x, 1, st))) return rc;
  if ((rc = psignn_plan_permute(p, prb, p->mixed ? 3 : 2, a.prb, 1, st))) return rc;
  return p->mixed ? psignn_plan_permute(p, nrm, 2, a.nrm, 1, st) : PSIGNN_OK;
}
static inline int psignn_from_plan(const psignn_plan* p, const float* src, float* dst, hipStream_t st) {
  return psignn_plan_permute(p, src, D, dst, 0, st);
}

// ---- the operator of an adjoint solve, y -> J_f(h*)^T y, set up once per solve (fgnn_layers.hip)
// Tiled plans: the whole solve in plan order -- h*, grad (x), prb and the normals are permuted into `rows` --; otherwise the
// caller's numbering.  Multi-layer dirichlet block: the layer states h_1..h_{L-1} at h* are evaluated once into lwork and each
// product runs the L backward layers only.  fwork: the f workspace the products use as scratch.
struct AdjointOp {
  const psignn_plan* p;
  const float *W, *h, *prb, *nrm, *grad;   // h*, prb, normals, grad: in the solve's numbering
  int nl;
  bool tiled, layers;
  float *fwork, *lwork;
  hipStream_t st;
  int setup(const psignn_plan* p, const float* W, int nl, const float* h_star, const float* prb, const float* nrm, const float* grad,
            ws::Adapter rows, float* fwork, float* lwork, hipStream_t st);
  int operator()(const float* y, float* out) const;
};
