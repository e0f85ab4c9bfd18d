// Launch shapes of the solver handles and the schedule of the Broyden update, described once (host only: no HIP header, compiles
// on its own; checked by tests/host/solver_shapes_check.cpp against tests/golden/broyden_schedule.json).
//
//   Knobs / knobs_from_env   the Broyden A/B knobs, read from the environment once per handle creation -- the only getenv of them
//   vec_shape                vector width, blocks, per-wave partials and row pitch of one vector (Broyden, fpiter, GMRES handles)
//   BroydenShape             everything psignn_broyden derives from its sizes and the knobs, with the bytes of every allocation
//   update_chain<Target>     which passes one iteration runs, with which arguments and stated bytes; a target launches them
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <algorithm>

#include "workspace.h"

namespace shapes {
constexpr int THREADS = 256;   // threads per block of the vector kernels (TB, vec_helpers.h)
constexpr int WAVE = 64;
constexpr size_t STATUS_BYTES = 88;   // sizeof(Status), solver.hip
constexpr int64_t VEC16_MIN = (int64_t)3 << 18;
inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
}  // namespace shapes

#define PARTA_LD 32            // row pitch of the folded sweep's partials: one entry per kept pair, so at most 32 kept pairs --
                               // U2R_KB_MAX + 1 = 25 in the register form, U2D_LDS_KMAX + 1 = 32 in the LDS form (k_sweep_u2d drops
                               // entries past the pitch, and k_reduce_a_check would read the next block's row in their place)
#define RA 8     // row chunks per column of the a-reduction: coef_a arrives as RA partial sums that sweep 2 adds up itself
#define U2R_KB_MAX 24
#define U2D_LDS_KMAX (PARTA_LD - 1)   // LDS form: k - j_keep0 + 1 <= PARTA_LD partials per row
static_assert(U2R_KB_MAX + 1 <= PARTA_LD, "the register fold's kept pairs must fit a partials row");

namespace shapes {
// ---- knobs: unset, or a value
struct Knob {
  bool set = false;
  int64_t v = 0;
};
struct Knobs {
  Knob vec16_min;   // PSIGNN_VEC16_MIN: elements from which the sweeps take 16 floats per lane -- of the Broyden handle only (broyden_shape);
                    // gmres_create (krylov.hip) and the fixed-point iteration handle (fpiter.hip) call vec_shape with the compiled-in
                    // VEC16_MIN, and a test selects their width with shard_elems (*_create_for_batch)
  Knob jgroups;     // PSIGNN_JGROUPS: pair groups of the split sweeps, 1 .. 8
  Knob vec_ax4;     // PSIGNN_VEC_AX4: 1 forces the 4-float unsplit axpy pass, 0 forbids it
  Knob uvu;         // PSIGNN_UVU: 0 forbids the three-sweep form
  Knob u2d_lds;     // PSIGNN_U2D_FORM: 1 = lds, 0 = anything else (registers)
  Knob u2d_kmax;    // PSIGNN_U2D_KMAX
  Knob u2d_keep;    // PSIGNN_U2D_KEEP
};
inline Knobs knobs_from_env() {
  Knobs k;
  auto num = [](const char* name, Knob& kn, bool wide) {
    if (const char* e = getenv(name)) kn = {true, wide ? (int64_t)atoll(e) : (int64_t)atoi(e)};
  };
  num("PSIGNN_VEC16_MIN", k.vec16_min, true);
  num("PSIGNN_JGROUPS", k.jgroups, false);
  num("PSIGNN_VEC_AX4", k.vec_ax4, false);
  num("PSIGNN_UVU", k.uvu, false);
  if (const char* e = getenv("PSIGNN_U2D_FORM")) k.u2d_lds = {true, (e[0] == 'l' || e[0] == 'L') ? 1 : 0};
  num("PSIGNN_U2D_KMAX", k.u2d_kmax, false);
  num("PSIGNN_U2D_KEEP", k.u2d_keep, false);
  return k;
}

// ---- one vector of n_elems elements, its width chosen for width_elems (its own length, or the whole shard's).
// 16 floats per lane from 768 K elements up, 4 below.  Re-tuned after the coalesced lane mapping, Broyden iterations/s with 4 vs
// 16 (dirichlet meshes, K = 100): 27 k nodes 12 790 / 10 156, 50 k 8 283 / 7 826, 100 k 4 578 / 4 972, 200 k 2 608 / 2 806,
// 400 k 1 416 / 1 551 (the old switch point was 4 M elements)
struct VecShape {
  int vec, nblk, npart;   // floats per lane, blocks, per-wave partials
  int64_t ld;             // row pitch: every stored vector starts on a 256-byte boundary (64 fp32 elements)
};
inline VecShape vec_shape(int64_t n_elems, int64_t width_elems, int64_t vec16_min = VEC16_MIN) {
  const int vec = width_elems >= vec16_min ? 16 : 4;
  const int nblk = (int)cdiv(n_elems, (int64_t)vec * THREADS);
  return {vec, nblk, nblk * (THREADS / WAVE), (n_elems + 63) / 64 * 64};
}

// ---- the Broyden solver
struct BroydenShape {
  int thr = 0;
  int vec = 16;             // elements per thread of the vector kernels
  int nblk = 0, npart = 0;
  int vec_ax = 0, nblk_ax = 0;  // axpy / final pass: own vector width on mid-size vectors
  int jgroups = 1;          // block rows of the U/V sweeps (short vectors are also split over the stored pairs)
  int uvu = 0;              // the update runs as three single-array sweeps U, V, U
  int vec_u = 0, nblk_u = 0, npart_u = 0;   // their vector width / blocks / per-wave partials per stored pair
  int u2d_kmax = 0, nblk4 = 0;  // folded sweep 3: up to this many stored pairs are all kept; its blocks
  int u2d_keep = 0;             // beyond u2d_kmax: the most recent u2d_keep pairs are kept
  int u2d_reg = 1;              // kept values in registers (k_sweep_u2r<KB>, the default) or in per-thread LDS slots (k_sweep_u2d)
  int nn_cap = 0;           // norm partial pairs: blocks of k_resid or tiles of the fused f kernel
  int ldp = 0;              // row pitch of a plane of dot partials: thr rounded up to 64
  int64_t pstride = 0;      // plane stride (floats): max blocks of any sweep form x ldp
  int64_t ld = 0;           // row pitch (elements) of U and V
  // bytes of every allocation, in the order they are made; jpart (scratch of a split axpy pass), fwork and the plan-order inputs
  // h0p, prbp, nrmp are 0 where the handle has none
  struct Bytes {
    size_t U, V, xbuf, gbuf0, gbuf1, upd, fx, part, parta, coef, st, nrm_part, part2, rel_trace, abs_trace;
    size_t jpart, fwork, h0p, prbp, nrmp;
    size_t total() const {
      return U + V + xbuf + gbuf0 + gbuf1 + upd + fx + part + parta + coef + st + nrm_part + part2 + rel_trace + abs_trace + jpart + fwork +
             h0p + prbp + nrmp;
    }
  } bytes = {};

  // does the fold need more than the default 64 KB of dynamic LDS?  (asked of the device lazily: only then)
  bool wants_big_lds() const { return u2d_kmax > 0 && !u2d_reg; }
  // not granted: stay within 64 KB (16 B x 256 threads x 15 pairs + the kernel's static 512 B)
  void cap_to_default_lds() {
    u2d_kmax = std::min(u2d_kmax, 15);
    u2d_keep = std::min(u2d_keep, 15);
  }
  // one size class: the vector width / split layout / threshold / fold limits that a shard's solvers must share
  bool same_size_class(const BroydenShape& b) const {
    return vec == b.vec && vec_ax == b.vec_ax && uvu == b.uvu && vec_u == b.vec_u && thr == b.thr && u2d_kmax == b.u2d_kmax &&
           u2d_keep == b.u2d_keep && u2d_reg == b.u2d_reg;
  }
};

// M elements; size_hint: elements of all vectors swept together (batched shard; 0: none); hist: 0 fp32 pairs, 1 bf16;
// plan_nodes / n_tiles: nodes and tiles of the handle's mesh plan (0 / 0 without a plan; an untiled plan has 0 tiles)
inline BroydenShape broyden_shape(int64_t M, int64_t size_hint, int thr, int hist, int keep_trace, int64_t plan_nodes, int64_t n_tiles,
                                  const Knobs& kn) {
  BroydenShape s;
  s.thr = thr;
  // A solver that will run inside a batched solve (size_hint = elements of the whole shard) sizes its sweeps for the
  // aggregate: the shard's blocks fill the chip together, so the long-vector width applies and the sweeps need no split
  // over the stored pairs.  Its single-mesh solves use the same shapes, hence the same bits as its batched ones.
  const int64_t eff = std::max<int64_t>(M, size_hint);
  const VecShape v = vec_shape(M, eff, kn.vec16_min.set ? kn.vec16_min.v : VEC16_MIN);
  s.vec = v.vec;
  s.nblk = v.nblk;
  const int64_t eff_blk = cdiv(eff, (int64_t)s.vec * THREADS);
  s.jgroups = eff_blk >= 768 ? 1 : (int)std::min<int64_t>(8, cdiv(768, eff_blk));
  // Shard of short vectors (8 x 50 k nodes: 123 blocks per mesh, 983 together): the chip is covered, but every block then walks
  // all stored pairs alone; the dots pass split 4 ways over the pairs and the axpy pass unsplit at 4 floats per lane
  // (3 930 blocks) measured 305 / 310 us against 325 / 313 us per launch (K = 100; profiles/r2_batch_sweep_ab.txt)
  const bool short_shard = size_hint > M && s.vec == 16 && s.nblk < 512;
  if (short_shard) s.jgroups = 4;
  if (kn.jgroups.set) s.jgroups = std::max(1, std::min(8, (int)kn.jgroups.v));   // A/B knob
  s.npart = v.npart;
  // Mid-size vectors (16 floats per lane, but too few blocks to fill the chip): the dots pass is split over the stored
  // pairs (free: every pair's partial sums are independent), the axpy pass would need a combine launch after such a split
  // -- it runs unsplit with 4 floats per lane instead (100 k nodes: 91 us vs 79 + 20 us).  The thread -> element mapping
  // is per kernel; only the pair partials that k_final reads must follow the axpy pass's block count.
  s.vec_ax = s.vec;
  s.nblk_ax = s.nblk;
  s.nblk4 = (int)cdiv(M, (int64_t)4 * THREADS);
  if (kn.vec_ax4.set ? (kn.vec_ax4.v != 0 && s.vec == 16) : (s.vec == 16 && s.jgroups > 1 && (short_shard || s.nblk4 >= 512))) {
    s.vec_ax = 4;
    s.nblk_ax = s.nblk4;
  }
  // three-sweep update (update_chain): where an UNSPLIT sweep covers the chip -- long vectors at 16 floats per lane, mid-size
  // vectors and shards of short vectors at the 4-float width of their axpy pass.  PSIGNN_UVU=0|1 overrides (A/B, tests).
  const bool long_form = s.vec == 16 && s.jgroups == 1 && s.vec_ax == 16;
  if (long_form) {
    s.uvu = 1; s.vec_u = 16; s.nblk_u = s.nblk;
  } else if (s.vec_ax == 4 && s.vec == 16) {
    s.uvu = 1; s.vec_u = 4; s.nblk_u = s.nblk_ax;
  }
  if (kn.uvu.set && kn.uvu.v == 0) s.uvu = 0;
  if (hist) {
    // bf16 pairs: always the unfolded three-sweep form (the two-pass form and the folded sweep 3 have no bf16 variant), 16 floats per
    // lane where the fp32 rules pick that width, else 4 floats unsplit; PSIGNN_UVU / PSIGNN_U2D_* do not apply
    s.uvu = 1;
    s.vec_u = long_form ? 16 : 4;
    s.nblk_u = (int)cdiv(M, (int64_t)s.vec_u * THREADS);
  }
  s.npart_u = s.nblk_u * (THREADS / WAVE);
  const bool fold_ok = s.uvu != 0;
  // folded sweep 3: kept values in registers (default; at most U2R_KB_MAX pairs) or in LDS (PSIGNN_U2D_FORM=lds: the round-2 form, A/B and tests)
  // Registers where the launch has several rounds of blocks (>= 2 048 blocks of 1 024 floats: 8 per CU); on shorter vectors every
  // block is resident at once, all waves then load together and reduce together, and the LDS form's two rounds overlap better
  // (100k nodes, K = 100: 56.5 vs 64.8 us per launch; profiles/r3_ab_u2d.txt).  M >= 2^30 floats: the register form's 32-bit lane
  // offsets do not reach.
  const bool reg_reaches = M < ((int64_t)1 << 30);
  s.u2d_reg = (kn.u2d_lds.set ? !kn.u2d_lds.v : cdiv(eff, (int64_t)4 * THREADS) >= 2048) && reg_reaches;
  // (LDS form: at most U2D_LDS_KMAX, so that k - keep0 + 1 kept pairs -- all k + 1 up to u2d_kmax, u2d_keep + 1 beyond -- fit PARTA_LD)
  const int kmax_cap = s.u2d_reg ? U2R_KB_MAX : U2D_LDS_KMAX;
  s.u2d_kmax = fold_ok ? 24 : 0;   // LDS form: 96 KB per block at most; 20 ... 32 measure alike at K = 50, K = 20 needs >= 19
  if (kn.u2d_kmax.set) s.u2d_kmax = fold_ok ? std::max(0, std::min(kmax_cap, (int)kn.u2d_kmax.v)) : 0;
  s.u2d_keep = s.u2d_kmax > 0 ? 16 : 0;
  if (kn.u2d_keep.set) s.u2d_keep = s.u2d_kmax > 0 ? std::max(0, std::min(s.u2d_kmax, (int)kn.u2d_keep.v)) : 0;
  if (hist) s.u2d_kmax = s.u2d_keep = 0;
  s.nn_cap = std::max<int>(std::max(s.nblk, s.nblk_ax), (int)n_tiles);
  s.ldp = (thr + 63) / 64 * 64;
  s.pstride = (int64_t)std::max(std::max(s.nblk, s.nblk_u), std::max(s.nblk_ax, 1)) * s.ldp;
  // row pitch of U and V: every stored vector starts on a 256-byte boundary (64 fp32 / 128 bf16 elements)
  s.ld = hist ? (M + 127) / 128 * 128 : v.ld;
  const size_t m4 = (size_t)M * 4, t = (size_t)thr, nx = keep_trace ? t + 2 : 3;
  const size_t pair = t * (size_t)s.ld * (hist ? 2 : 4);   // U, V: bytes per stored pair element
  const bool split_axpy = s.jgroups > 1 && s.vec_ax == s.vec;
  const size_t N = (size_t)plan_nodes;
  s.bytes = {pair, pair, nx * m4, m4, m4, m4, m4, 3 * (size_t)s.pstride * 4 + 16, (size_t)s.nblk4 * PARTA_LD * 4 + 16,
             (3 + RA) * t * 4 + 16, STATUS_BYTES, 2 * (size_t)s.nn_cap * 4 + 16, 2 * (size_t)std::max(s.nblk, s.nblk_u) * 4 + 16, t * 8 + 8,
             t * 8 + 8,
             split_axpy ? (size_t)s.jgroups * 3 * m4 : 0, N ? (size_t)ws::f_total(plan_nodes) * 4 : 0, N ? m4 : 0, N * 3 * 4, N * 2 * 4};
  return s;
}

// ------------------------------------------------------------------------------------------
// The update chain: everything of one iteration after g_new and the norm partials are available; k = pairs stored so far.
// The schedule stands here once -- two-pass or three-sweep form, which a_j the folded sweep 3 of the last iteration delivered
// (a_ready / a_from), the keep window and its KB, LDS or register fold, the `last` gate, the split over pair groups with its combine
// launch, the own-width axpy pass, and the algorithmic bytes of every launch (t.bytes(b): of the pass issued next).  A target knows
// HOW a pass is launched: SingleTarget (the k_* kernels on one solver's fields) and ShardTarget (the kb_* kernels, one launch per pass
// over a shard) in solver.hip, the recording target of tests/host/solver_shapes_check.cpp.
// ------------------------------------------------------------------------------------------
template <class Target>
static void update_chain(Target& t, int k, double eps) {
  const BroydenShape& c = t.size_class();
  const int thr = c.thr;
  const int64_t vb = t.vec_bytes();                    // one state vector (summed over a shard)
  const int64_t pe = vb / 4 * t.pair_elem_bytes();     // one stored vector U_j / V_j
  const int kd = k >= thr ? 0 : k;   // the threshold stop is about to fire: no slot left for another pair
  const bool last = k + 1 >= thr;    // (iteration thr's stop test has just fired: the passes after it return at once and state no bytes)
  if (c.uvu) {
    if (k == 0) t.a_ready() = 0;
    // a_j of this iteration: pairs j >= a_from were delivered by the folded sweep 3 of the last iteration, the others need sweep 1
    // (all meshes of a shard carry the same number of stored pairs: one a_from / keep window for the launch)
    const int a_from = t.a_ready() ? t.a_from() : kd;
    const int n1 = std::min(a_from, kd);
    if (n1 > 0) {
      t.bytes(n1 * pe + vb);   // its columns of U + dx
      t.sweep_u1(n1);
    }
    t.reduce_a_check(kd, eps, a_from);
    t.a_ready() = 0;
    if (k >= thr) return;
    t.bytes(last ? 0 : (k + 1) * pe + 3 * vb);   // k columns of V + dx, dg, g; writes V[k]
    t.sweep_v(k);
    t.reduce_cb(k);
    const int keep0 = k <= c.u2d_kmax ? 0 : k - c.u2d_keep;      // few stored pairs: all kept; later the most recent ones
    if (c.u2d_kmax > 0 && (k <= c.u2d_kmax || c.u2d_keep > 0) && !last) {
      t.bytes((k + 1) * pe + 4 * vb);   // k columns of U + update, dg, g; writes U[k], update (whichever form runs)
      const int nk = k - keep0;
      if (!c.u2d_reg) t.sweep_u2d(k, keep0, (size_t)std::max(nk, 1) * THREADS * 16);
      else if (nk <= 8) t.template sweep_u2r<8>(k, keep0);
      else if (nk <= 16) t.template sweep_u2r<16>(k, keep0);
      else t.template sweep_u2r<24>(k, keep0);
      t.a_ready() = 1;
      t.a_from() = keep0;
    } else {
      t.bytes(last ? 0 : (k + 1) * pe + 4 * vb);
      t.sweep_u2(k);
    }
    return;
  }
  // split of the sweeps over the stored pairs: only when there are enough pairs to share out
  const int G = t.groups(k);
  if (kd > 0) {
    t.bytes((2 * kd + 3) * vb);
    t.dots(kd, G);
  }
  t.reduce_check(kd, eps);
  if (k >= thr) return;
  const bool own_width = c.vec_ax != c.vec;   // the axpy / final passes run unsplit at their own vector width (broyden_shape)
  const int Ga = own_width ? 1 : G;
  t.bytes(last ? 0 : (2 * k + (Ga > 1 ? 3 * Ga : 6)) * vb);   // split: every block row writes its three partial vectors
  t.axpy(k, Ga, own_width);
  if (!own_width && t.combine_due(k, G)) {
    t.bytes(last || G <= 1 ? 0 : (3 * G + 6) * vb);
    t.combine(k, G);
  }
  t.bytes(last ? 0 : 4 * vb);
  t.final_pass(k, own_width);
}
}  // namespace shapes
