// Every device workspace of the library, described once (host only: no HIP header, compiles on its own).
//
// A layout is a plain struct of named segments (floats) and `total`, filled by one builder.  With base == nullptr the builder only
// sizes: the *_workspace_floats queries return that total and the entry points carve the caller's buffer with the same builder,
// so the size and the layout cannot disagree.  Segments follow each other in the order of the struct, without padding, unless a
// comment declares an alias.  Where a query promises more than the layout uses, the difference is the trailing `spare`.  A
// builder with a `total` argument carves a region of that many floats (0: as much as it uses) inside another layout.
#pragma once
#include <stdint.h>

#ifndef PSIGNN_D
#define PSIGNN_D 10
#endif

namespace ws {
constexpr int64_t W = PSIGNN_D;   // one latent row

// Parameter-gradient records (static_assert'ed against the Tab* structs of fgnn_pgrad.hip): floats of one node's record and
// 16 x 16 accumulator tiles of each table.  LAYER_VIEW: a single-layer view of the weights (fgnn_layers.hip).
constexpr int64_t REC_F = 320, REC_X = 480, REC_G = 320, REC_GX = 480, REC_M = 64, LAYER_VIEW = 4096;
constexpr int NT_F = 16, NT_X = 24, NT_G = 19, NT_GX = 27, NT_M = 2;
constexpr int rec_f(bool mixed) { return (int)(mixed ? REC_X : REC_F); }   // floats of one f_theta record on a plan of that family

struct Carve {
  float* base;
  int64_t o = 0;
  float* take(int64_t n) {
    float* q = base ? base + o : nullptr;
    o += n;
    return q;
  }
  float* rest(int64_t total) { return take(total > o ? total - o : 0); }   // up to the end of a region of `total` floats
  void even() { o += o & 1; }
  template <class T> T done(T w) const { w.total = o; return w; }   // a layout whose segments are carved: its total
};

// Block count of k_pgrad_outer over n_rec records: a wave owns >= 64 records (a multiple of 4), at most 1024 blocks of 4 waves
inline int pgrad_blocks(int64_t n_rec, int* per_wave) {
  int64_t npw = ((n_rec + 4095) / 4096 + 3) / 4 * 4;
  if (npw < 64) npw = 64;
  *per_wave = (int)npw;
  return (int)((n_rec + npw * 4 - 1) / (npw * 4));
}
// Partial tiles of the reduction of n_rec records with a table of nt tiles: one set per block while four waves' tiles fit in LDS
// (nt <= 16), one per wave beyond
inline int64_t pg_part(int64_t n_rec, int nt) {
  int npw;
  return (int64_t)pgrad_blocks(n_rec, &npw) * (nt <= 16 ? 1 : 4) * nt * 256;
}

// ---- f workspace (psignn_f_workspace_floats): N * 10 rows, read through one of these views
inline int64_t f_total(int64_t N) { return N * 10 * W; }

// forward / JVP: Pj (gather kernels: value and tangent projections, up to 3 Phi modules; tile kernels: empty) | the two ping-pong
// rows of a multi-layer block.  total: the region it is carved from
struct FFwd { float *Pj, *pp[2], *spare; int64_t total; };
inline FFwd f_fwd(int64_t N, bool tiles, float* base, int64_t total) {
  Carve c{base};
  return c.done(FFwd{c.take(tiles ? 0 : N * 6 * W), {c.take(N * W), c.take(N * W)}, c.rest(total), 0});
}
// gather VJP: Pj (N, 2 W | 3 W) | B (N, 4 W | 6 W).  (The tile VJP takes B (N, 4 W) alone: the first segment of what it is given.)
struct FVjp { float *Pj, *B, *spare; int64_t total; };
inline FVjp f_vjp(int64_t N, bool mixed, float* base, int64_t total) {
  Carve c{base};
  return c.done(FVjp{c.take(N * (mixed ? 3 : 2) * W), c.take(N * (mixed ? 6 : 4) * W), c.rest(total), 0});
}
// Caller-order adapter of a tiled plan: plan-order copies of the caller's tensors around a plan-order kernel.
//   [ B (N, 4 W): the tile VJP's scratch, VJP only ] | h | x | out | prb (N, prb_cols) | nrm (N, 2) | rest
// x: h_initial (forward), the tangent (JVP), the cotangent (VJP, parameter VJP).  nrm starts on an even offset; rest on a
// multiple of four where rows behind it are read as float4 (rest_quad).  rest: what the kernel behind the adapter carves.
// f_adapter: over the f workspace, where prb takes 3 columns whatever the family.
struct Adapter { float *B, *h, *x, *out, *prb, *nrm, *rest; int64_t rest_floats, total; };
inline Adapter adapter(int64_t N, bool with_B, int prb_cols, bool with_nrm, bool rest_quad, float* base, int64_t total) {
  Carve c{base};
  Adapter w{c.take(with_B ? N * 4 * W : 0), c.take(N * W), c.take(N * W), c.take(N * W), c.take(N * prb_cols)};
  c.even();
  w.nrm = c.take(with_nrm ? N * 2 : 0);
  if (rest_quad) c.o += (4 - (c.o & 3)) & 3;
  w.rest_floats = total - c.o;
  w.rest = c.rest(total);
  return c.done(w);
}
inline Adapter f_adapter(int64_t N, bool with_B, float* base) { return adapter(N, with_B, 3, true, false, base, f_total(N)); }

// The Broyden adjoint solve on a tiled plan keeps h* (h) and grad in plan order (x) in its own f workspace where the VJP adapter
// does: behind B, the scratch of the tile VJP -- the operator is given the whole workspace and uses those first N * 4 W floats.
// (prb and nrm: the solver's own rows.)
inline Adapter f_adjoint(int64_t N, float* base) { return f_adapter(N, true, base); }

// ---- layer workspace of a multi-layer block (psignn_f_layers_workspace_floats): 4 L + 1 rows | a single-layer weight view; a
// mixed block differentiates its last layer only: the view alone.  Two readings of the rows, never both in one call:
//   chains (JVP, VJP, parameter VJP):  h_1..h_{L-1} | t_a | t_b | init (the h_initial cotangent in plan order)
//   backward of the VJP:               h_1..h_{L-1} | w_1..w_{L-1} | gbar_1..gbar_{L-1} | c_0..c_{L-1} | a (2) | prod
struct LayerWork {
  float *S, *tb[2], *init;     // states; chains
  float *Wc, *G, *C, *A, *T;   // backward of the VJP: alias tb, init and the rows behind them
  float *spare, *view;
  int64_t ND, total;
  float* row(float* seg, int k) const { return seg + k * ND; }
  float* state(int k) const { return row(S, k - 1); }   // h_k, 1 <= k <= L - 1
};
inline LayerWork layer_work(int64_t N, int nl, bool mixed, float* base) {
  Carve c{base};
  LayerWork w{};
  const int64_t ND = w.ND = N * W;
  if (nl > 1 && !mixed) {
    w.S = c.take((nl - 1) * ND);
    Carve b = c;   // the second reading starts where the first does
    w.tb[0] = c.take(ND); w.tb[1] = c.take(ND); w.init = c.take(ND);
    w.Wc = b.take((nl - 1) * ND); w.G = b.take((nl - 1) * ND); w.C = b.take(nl * ND); w.A = b.take(2 * ND); w.T = b.take(ND);
    if (b.o > c.o) c.o = b.o;
    w.spare = c.rest((4 * nl + 1) * ND);
  }
  w.view = c.take(nl > 1 ? LAYER_VIEW : 0);
  return c.done(w);
}

// ---- scratch | records | partial tiles: the parameter VJP, the DS-GPS / DSS step backward, the MLP backward
struct RecWork { float *scratch, *rec, *part, *spare; int64_t total; };
inline RecWork rec_work(int64_t scratch, int64_t rec, int64_t part, float* base, int64_t total) {
  Carve c{base};
  return c.done(RecWork{c.take(scratch), c.take(rec), c.take(part), c.rest(total), 0});
}
// parameter VJP (psignn_f_param_vjp_workspace_floats): sized for the mixed family behind a caller-order adapter.
// scratch_rows = 4: the tile VJP's B alone (single-layer tiled plans); 9: room for the gather VJP's Pj | B (f_vjp), which the
// layer chains keep on tiled plans too.
inline int64_t pv_total(int64_t N) { return N * (9 * W + 36 + REC_X) + pg_part(N, NT_X); }
inline RecWork pv_work(int64_t N, bool mixed, int scratch_rows, float* base, int64_t total) {
  return rec_work(N * scratch_rows * W, N * (mixed ? REC_X : REC_F), pg_part(N, mixed ? NT_X : NT_F), base, total);
}
inline Adapter pv_adapter(int64_t N, bool mixed, float* base) { return adapter(N, false, mixed ? 3 : 2, mixed, true, base, pv_total(N)); }
// step backward of DS-GPS (scratch: jr_scratch; sized for the mixed family) and DSS, backward of the two-layer MLP
inline RecWork dsgps_bw_work(int64_t N, bool mixed, float* base) {
  return rec_work(N * 17 * W, N * (mixed ? REC_GX : REC_G), pg_part(N, mixed ? NT_GX : NT_G), base, N * (17 * W + REC_GX) + pg_part(N, NT_GX));
}
inline RecWork dss_bw_work(int64_t N, float* base) { return rec_work(N * 13 * W, N * REC_F, pg_part(N, NT_F), base, 0); }
inline RecWork mlp2_bw_work(int64_t n, float* base) { return rec_work(0, n * REC_M, pg_part(n, NT_M), base, 0); }

// scratch of the gather kernels of gather_backward.hip: P (N, 4 W | 6 W) | cb (N, 4 W) | B (N, 4 W | 6 W) | dir (N, W)
struct JrScratch { float *P, *cb, *B, *dir; int64_t total; };
inline JrScratch jr_scratch(int64_t N, bool mixed, float* base) {
  Carve c{base};
  return c.done(JrScratch{c.take(N * (mixed ? 6 : 4) * W), c.take(N * 4 * W), c.take(N * (mixed ? 6 : 4) * W), c.take(N * W), 0});
}
// ---- backward of the VJP, gather form (psignn_f_vjp_backward_workspace_floats; sized for the mixed family):
//   scratch (jr_scratch; N * 17 W) | rec1 | rec2 | part2 | spare      followed, for n_layers > 1, by the layer workspace
// part1: the partial tiles of the chain-back pass of a multi-layer dirichlet block, which leaves ONE record set (rec1): they start
// where rec2 does and may run over it into part2 -- neither is live then.
// The plan-order tile form (psignn_f_vjp_backward_p_workspace_floats; dirichlet): scratch = the tile kernels' B (N, 6 W), no spare.
struct JrWork { float *scratch, *rec1, *rec2, *part2, *spare, *part1 /* alias: rec2 onwards */; int64_t total; };
inline JrWork jr_work(int64_t N, bool mixed, bool tiles, float* base) {
  Carve c{base};
  const int64_t rec = N * (mixed ? REC_X : REC_F);
  JrWork w{c.take(N * (tiles ? 6 : 17) * W), c.take(rec), c.take(rec), c.take(pg_part(2 * N, mixed ? NT_X : NT_F)),
           c.rest(tiles ? 0 : N * (17 * W + 2 * REC_X) + pg_part(2 * N, NT_X))};
  w.part1 = w.rec2;
  return c.done(w);
}

// ---- DS-GPS / DSS forward, caller order (no size query: the documented sizes are N * 4 W and N * (2 W + 3))
struct DsgpsWork { float *h0, *a, *b, *prb, *nrm, *spare; int64_t total; };
inline DsgpsWork dsgps_work(int64_t N, bool mixed, float* base) {
  Carve c{base};
  DsgpsWork w{c.take(N * W), c.take(N * W), c.take(N * W), c.take(N * (mixed ? 3 : 2))};
  c.even();
  w.nrm = c.take(mixed ? N * 2 : 0);
  w.spare = c.rest(N * 4 * W);
  return c.done(w);
}
struct DssWork { float *a, *b, *bprime; int64_t total; };
inline DssWork dss_work(int64_t N, float* base) {
  Carve c{base};
  return c.done(DssWork{c.take(N * W), c.take(N * W), c.take(N * 3), 0});
}

// ---- GMRES adjoint solve (psignn_gmres_adjoint_workspace_floats); segments start on 256-byte boundaries
//   operator scratch | y | J^T y | y_best | grad_p | h*_p | prb_p | normals_p | layer states
struct AdjWork { float *fwork, *y, *fy, *ybest, *grad_p, *hs_p, *prbp, *nrmp, *lwork; int64_t total; };
inline AdjWork adj_work(int64_t N, int nl, bool mixed, float* base) {
  const int64_t M = N * W;
  Carve c{base};
  auto take = [&](int64_t n) { return c.take((n + 63) / 64 * 64); };
  return c.done(AdjWork{take(f_total(N)), take(M), take(M), take(M), take(M), take(M), take(N * 3), take(N * 2),
                        take(mixed ? 0 : layer_work(N, nl, false, nullptr).total), 0});   // the operator of a mixed block needs no layer states
}

// ---- float64 mean-square error (psignn_mse_f64_workspace_doubles; DOUBLES, one segment): one partial per chunk of MSE64_CHUNK
// elements, in chunk order; one block then adds them (poisson_cg.hip)
constexpr int64_t MSE64_CHUNK = 1024;
inline int64_t mse64_total(int64_t n_elems) { return (n_elems + MSE64_CHUNK - 1) / MSE64_CHUNK; }

// ---- float64 Newton-Krylov (psignn_gmres64_solve_shifted, psignn_newton64_solve; DOUBLES)
// The caller's product workspace: one region that either product carves as psignn_f64_deriv_workspace_doubles describes it -- the
// larger of the J v and the J^T w counts (the solve runs one orientation per call).
inline int64_t shifted64_total(int64_t jvp_doubles, int64_t vjp_doubles) { return jvp_doubles > vjp_doubles ? jvp_doubles : vjp_doubles; }
// The Newton handle's own state, M = N * W doubles each, in this order, without padding:
//   x | f(x) | g = f(x) - x | x_t (the trial point) | f(x_t) | delta (the step; g(x_t) once x_t is formed)
// An accepted step swaps the roles of (x, f(x), g) and (x_t, f(x_t), delta); a rejected one writes only the last three.
struct Newton64Vecs { double *x, *fx, *g, *xt, *fxt, *delta; int64_t total; };
inline Newton64Vecs newton64_vecs(int64_t N, double* base) {
  const int64_t M = N * W;
  auto at = [&](int64_t k) { return base ? base + k * M : nullptr; };
  return Newton64Vecs{at(0), at(1), at(2), at(3), at(4), at(5), 6 * M};
}
}  // namespace ws
