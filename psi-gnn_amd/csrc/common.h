// Shared declarations for libpsignn_hip (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string>
#include "../../include/psignn_hip.h"

#define D PSIGNN_D
// The latent width is a compile-time constant.  libpsignn_hip.so is built for 10 (every derivative kernel exists at that width
// only); libpsignn_hip_d<w>.so compiles the forward translation units again for another even width (Makefile).  Rows of D floats
// move as D/2 float2 (global) or as 16-byte quads (LDS), and the packed-fp32 node arithmetic holds a row as NPAIR = D/2 register
// pairs -- hence even; the upper bound keeps the row arrays of the tile kernel (8 live NPAIR-pair vectors) inside the register file.
static_assert(D % 2 == 0 && D >= 4 && D <= 16, "PSIGNN_D: an even latent width from 4 to 16");
#define NPAIR (D / 2)   // register pairs of one latent row

void psignn_set_error(const char* fmt, ...);

// Run-time knobs (PSIGNN_* environment variables; A/B scaffolding and test selectors, never needed for a normal run) are read
// once and cached; psignn_reload_knobs() bumps the epoch so that the next use re-reads them (tests switch forms in-process).
extern int g_knob_epoch;
#define KNOB_INT(var, expr)                   \
  static int var##_epoch = -1;                \
  static int var = 0;                         \
  if (var##_epoch != g_knob_epoch) {          \
    var = (expr);                             \
    var##_epoch = g_knob_epoch;               \
  }

#define HIP_TRY(expr)                                                                   \
  do {                                                                                  \
    hipError_t _e = (expr);                                                             \
    if (_e != hipSuccess) {                                                             \
      psignn_set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e)); \
      return PSIGNN_EHIP;                                                               \
    }                                                                                   \
  } while (0)
// HIP_TRY with another way out: a create function passes the call that destroys its half-built handle and yields the code.
// (Not HIP_TRY's body: an argument handed on to a second macro is expanded before # sees it, which would change the messages.)
#define HIP_TRY_OR(expr, on_fail)                                                       \
  do {                                                                                  \
    hipError_t _e = (expr);                                                             \
    if (_e != hipSuccess) {                                                             \
      psignn_set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e)); \
      return (on_fail);                                                                 \
    }                                                                                   \
  } while (0)

// who: the entry point the message names (an implementation shared by two entry points passes the one that was called)
#define ARG_CHECK_AS(who, cond, msg)                           \
  do {                                                         \
    if (!(cond)) {                                             \
      psignn_set_error("%s: %s", who, msg);                    \
      return PSIGNN_EINVAL;                                    \
    }                                                          \
  } while (0)
#define ARG_CHECK(cond, msg) ARG_CHECK_AS(__func__, cond, msg)

static inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// Owner of one array for the span of a call: alloc(n) once, get(), freed by the destructor -- so that HIP_TRY and `return rc` may
// leave the function anywhere.  Neither copyable nor movable.
template <class T, hipError_t (*Alloc)(void**, size_t), hipError_t (*Free)(void*)>
class ScopedArray {
 public:
  ScopedArray() = default;
  ScopedArray(const ScopedArray&) = delete;
  ScopedArray& operator=(const ScopedArray&) = delete;
  ~ScopedArray() { if (p_) (void)Free(p_); }
  hipError_t alloc(size_t n) {
    if (p_) return hipErrorInvalidValue;
    const hipError_t e = Alloc(reinterpret_cast<void**>(&p_), n * sizeof(T));
    if (e != hipSuccess) p_ = nullptr;
    return e;
  }
  T* get() const { return p_; }

 private:
  T* p_ = nullptr;
};
static inline hipError_t device_alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
static inline hipError_t device_free(void* p) { return hipFree(p); }
static inline hipError_t pinned_alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes); }
static inline hipError_t pinned_free(void* p) { return hipHostFree(p); }
template <class T> using DeviceArray = ScopedArray<T, device_alloc, device_free>;   // device memory
template <class T> using PinnedArray = ScopedArray<T, pinned_alloc, pinned_free>;   // pinned host memory

// Copy n descriptors to the device and wait: they are read from pageable host memory, which must have left the host before its
// owner can go.
template <class T>
static inline int upload_wait(T* d_dst, const T* h_src, size_t n, hipStream_t st) {
  HIP_TRY(hipMemcpyAsync(d_dst, h_src, sizeof(T) * n, hipMemcpyHostToDevice, st));
  HIP_TRY(hipStreamSynchronize(st));
  return PSIGNN_OK;
}

// ---------------------------------------------------------------------------------------------
// Weight pack layout (floats).  All blocks are nn.Linear (out,in) row-major.
// Written for D = 10 (the numbers in brackets); every size and offset is an expression in D:
//   shared : ln_gamma[D] ln_beta[D] alpha_w[3D+P] alpha_b[1]              (padded to SHARED_SZ, a multiple of 16: 64)
//   layer l: phi_to{W1[10x23] b1[10] W2[10x10] b2[10]}  phi_from{...}  update{U1[10x(30+P)] c1[10] U2[10x10] c2[10]}
//            fold{G_to[10x10] g_to[10] G_fr[10x10] g_fr[10] a_to[10] a_fr[10] ab_to ab_fr}          (FOLD_SZ 244: padded to 4)
//   mixed  : phi_neu{...350}  upd_neu{N1[10x25] n1[10] N2[10x10] n2[10]}  nfold{G_n[10x10] g_n[10]} (NFOLD_SZ 112: padded to 4)
// P = second_member_dim = 2 (dirichlet) / 3 (mixed).
// fold blocks are derived on the host (engine.pack_weights): the second Phi layer is linear, so
//   U1[:, mp_to cols] (W2_to S + deg b2_to) = G_to S + deg g_to   with G_to = U1_to W2_to, g_to = U1_to b2_to
// and likewise for the alpha gate (a_to = w_alpha,to W2_to, ab_to = w_alpha,to . b2_to) and the Neumann MLP.
// ---------------------------------------------------------------------------------------------
template <int P>
struct WLayout {
  static constexpr int CAT = 3 * D + P;       // 32 / 33
  static constexpr int EIN = 2 * D + 3;       // 23
  static constexpr int LN_G = 0, LN_B = D, AL_W = 2 * D, AL_B = 2 * D + CAT;
  static constexpr int SHARED_SZ = (2 * D + 3 * D + 3 + 1 + 15) / 16 * 16;   // sized for P = 3 in both families: 64
  static constexpr int PHI_SZ = D * EIN + D + D * D + D;  // 350
  static constexpr int PHI_W1 = 0, PHI_B1 = D * EIN, PHI_W2 = D * EIN + D, PHI_B2 = D * EIN + D + D * D;
  static constexpr int UPD_SZ = D * CAT + D + D * D + D;
  static constexpr int UPD_W1 = 0, UPD_B1 = D * CAT, UPD_W2 = D * CAT + D, UPD_B2 = D * CAT + D + D * D;
  static constexpr int F_GTO = 0, F_gTO = D * D, F_GFR = D * D + D, F_gFR = 2 * D * D + D, F_ATO = 2 * D * D + 2 * D,
                       F_AFR = 2 * D * D + 3 * D, F_ABTO = 2 * D * D + 4 * D, F_ABFR = 2 * D * D + 4 * D + 1;
  static constexpr int FOLD_SZ = (2 * D * D + 4 * D + 2 + 3) / 4 * 4;
  static constexpr int LAYER_SZ = 2 * PHI_SZ + UPD_SZ + FOLD_SZ;
  static constexpr int L_TO = 0, L_FROM = PHI_SZ, L_UPD = 2 * PHI_SZ, L_FOLD = 2 * PHI_SZ + UPD_SZ;
  static constexpr int NFOLD_SZ = (D * D + D + 3) / 4 * 4, NF_G = 0, NF_g = D * D;
  static constexpr int NEU_CAT = 2 * D + P + 2;  // 25 (mixed only)
  static constexpr int NEU_SZ = D * NEU_CAT + D + D * D + D;
  static constexpr int NEU_W1 = 0, NEU_B1 = D * NEU_CAT, NEU_W2 = D * NEU_CAT + D, NEU_B2 = D * NEU_CAT + D + D * D;
  __host__ __device__ static constexpr int layer(int l) { return SHARED_SZ + l * LAYER_SZ; }
  __host__ __device__ static constexpr int phi_neu(int nl) { return SHARED_SZ + nl * LAYER_SZ; }
  __host__ __device__ static constexpr int upd_neu(int nl) { return SHARED_SZ + nl * LAYER_SZ + PHI_SZ; }
  __host__ __device__ static constexpr int nfold(int nl) { return SHARED_SZ + nl * LAYER_SZ + PHI_SZ + NEU_SZ; }
  __host__ __device__ static constexpr int base_total(int nl, bool mixed) {
    return SHARED_SZ + nl * LAYER_SZ + (mixed ? PHI_SZ + NEU_SZ + NFOLD_SZ : 0);
  }
  // ---- transposed section (tile kernel): every matrix again as [in k][out o], o fastest, so that the outputs
  // (o, o+1) of one input k are adjacent -> one SGPR pair feeds a v_pk_fma_f32.  FP32 peak on CDNA needs the
  // packed form; the scalar form issues at half the rate.  Derived on the host (engine.pack_weights).
  // Blocks: D x D matrices, 3 x D edge-attr blocks, D-vectors; U1P / N1P hold 3 / 5 input rows in both families (P <= 3).
  static constexpr int DD = D * D;
  static constexpr int T_W1J_TO = 0, T_W1J_FR = DD, T_W1I_TO = 2 * DD, T_W1I_FR = 3 * DD, T_A_TO = 4 * DD,
                       T_A_FR = T_A_TO + 3 * D, T_B1_TO = T_A_FR + 3 * D, T_B1_FR = T_B1_TO + D, T_U1H = T_B1_FR + D,
                       T_GTO = T_U1H + DD, T_GFR = T_GTO + DD, T_U1P = T_GFR + DD, T_HB = T_U1P + 3 * D, T_gTO = T_HB + D,
                       T_gFR = T_gTO + D, T_U2 = T_gFR + D, T_C2 = T_U2 + DD, TPL_SZ = T_C2 + D;
  static constexpr int N_W1J = 0, N_W1I = DD, N_A = 2 * DD, N_B1 = N_A + 3 * D, N_N1H = N_B1 + D, N_GN = N_N1H + DD,
                       N_N1P = N_GN + DD, N_NB1 = N_N1P + 5 * D, N_gN = N_NB1 + D, N_N2 = N_gN + D, N_NB2 = N_N2 + DD,
                       TPN_SZ = N_NB2 + D;
  __host__ __device__ static constexpr int tp_layer(int nl, bool mixed, int l) { return base_total(nl, mixed) + l * TPL_SZ; }
  __host__ __device__ static constexpr int tp_neu(int nl) { return base_total(nl, true) + nl * TPL_SZ; }
  __host__ __device__ static constexpr int total(int nl, bool mixed) {
    return base_total(nl, mixed) + nl * TPL_SZ + (mixed ? TPN_SZ : 0);
  }
};
#if PSIGNN_D == 10   // the layout every derivative kernel, test and stored profile was written against
static_assert(WLayout<2>::SHARED_SZ == 64 && WLayout<3>::AL_B == 53 && WLayout<2>::PHI_SZ == 350 && WLayout<2>::FOLD_SZ == 244 &&
              WLayout<2>::F_ABFR == 241 && WLayout<3>::NFOLD_SZ == 112 && WLayout<2>::LAYER_SZ == 1384 && WLayout<3>::LAYER_SZ == 1394 &&
              WLayout<2>::T_U1P == 780 && WLayout<2>::T_C2 == 940 && WLayout<2>::TPL_SZ == 950 && WLayout<3>::N_NB1 == 490 &&
              WLayout<3>::TPN_SZ == 620 && WLayout<2>::total(1, false) == 2398 && WLayout<3>::total(1, true) == 3860,
              "weight layout at D = 10");
#endif
// every block of the transposed section starts on an 8-byte boundary (read as float2 pairs)
static_assert(WLayout<2>::total(1, false) % 2 == 0 && WLayout<3>::base_total(1, true) % 2 == 0 && WLayout<2>::LAYER_SZ % 2 == 0,
              "transposed weight blocks are read as float2");

// Iteration-invariant pointers of a tiled plan, kept in DEVICE memory and handed to the tile kernels as one pointer.
// As separate kernel arguments they are all live from the kernel's first instruction; the f kernel needs ~60 SGPRs for
// weights in its hot phases, so the compiler parked those arguments in VGPR lanes (v_writelane / v_readlane: VALU issue
// slots).  Behind a pointer each one is a scalar load next to its use.
struct TileCtx {
  const int32_t *tile_ptr, *tile_slice, *halo, *halo_cnt, *slice_off;
  const uint8_t* slice_deg;
  const uint4* ell;
  const uint8_t* flags_p;
  // tiles are consecutive chunks of `tile_nodes` nodes (a multiple of 64; the last tile may be short): a tile's node range and
  // its first slice follow from its index -- no dependent scalar load in front of the kernel's first vector loads
  int32_t tile_nodes;
  int32_t n_nodes;
};

// ---------------------------------------------------------------------------------------------
// Mesh plan (device memory owned here).
// ---------------------------------------------------------------------------------------------
struct psignn_plan {
  int64_t N = 0, E = 0, Ep = 0;
  int mixed = 0;
  int32_t *csr_ptr = nullptr, *csr_nbr = nullptr, *csr_eid = nullptr;
  int32_t *csc_ptr = nullptr, *csc_nbr = nullptr, *csc_eid = nullptr;
  float *csr_attr = nullptr, *csc_attr = nullptr;  // (E',3)
  uint8_t* flags = nullptr;                        // (N)
  int32_t *a_ptr = nullptr, *a_col = nullptr;      // full CSR of A (self loops included)
  float* a_val = nullptr;
  int32_t* a_eid = nullptr;                        // (E) original edge id of every full-CSR entry (poisson_cg.hip gathers its fp64 values by it)
  int max_deg = 0;

  // ---- tile structures (tiles.hip); valid when tiled != 0 -------------------------------------
  // Nodes are renumbered so that a tile (<= TILE_MAX consecutive new ids) is spatially compact; a tile's
  // out-of-tile neighbours form its halo.  Solver state lives in the new ("plan") order.
  int tiled = 0;
  int64_t n_tiles = 0, n_slices = 0, ell_rows = 0;
  int max_rows = 0;                            // max over tiles of n_t + n_halo (LDS rows)
  int32_t *perm = nullptr, *inv = nullptr;     // perm[new] = old ; inv[old] = new
  int32_t* tile_ptr = nullptr;                 // (n_tiles+1) new-id ranges
  int32_t* tile_slice = nullptr;               // (n_tiles+1) first 64-lane slice of each tile
  int32_t *halo = nullptr, *halo_cnt = nullptr;  // (n_tiles, HALO_CAP) sorted new ids ; (n_tiles)
  int32_t* slice_off = nullptr;                // (n_slices+1) first ELL slot-row of each slice
  uint8_t* slice_deg = nullptr;                // (n_slices) slot-rows of the slice (max neighbour slots of its nodes)
  uint4* ell = nullptr;                        // (ell_rows, 64) pair-merged slots {row|IN|OUT, a0, a1, a2}, tiles.hip
  uint8_t* flags_p = nullptr;                  // node flags in plan order
  // mixed plans: tiles without Neumann nodes first, then the (few, boundary) tiles with Neumann nodes -- the f kernel
  // runs the first group without the Phi_neumann columns in LDS (80-byte rows, one more workgroup per CU)
  int32_t* tile_order = nullptr;               // (n_tiles) tile ids
  int64_t n_tiles_plain = 0;                   // tiles in the first group
  float cell_size = 0.f, xmin = 0.f, ymin = 0.f;
  int nx = 0, ny = 0;
  TileCtx* d_ctx = nullptr;                    // device copy of the tile pointers (the batched fused step's mesh descriptors)
  TileCtx h_ctx{};                             // the same on the host (kernels that take the struct by value)
};


#define TILE_MAX 256      // nodes per tile = threads per block of the tile kernel
#define HALO_CAP 512      // halo entries stored per tile
// Mixed plans: tile + halo rows at most 682, the 240-byte LDS rows of the Neumann tiles' JVP (k_jvp_tile) in 160 KiB.
// The tile builder keeps a mixed plan with more rows untiled, so that every tile kernel runs on every tiled plan.
#define MIXED_ROW_CAP (160 * 1024 / (60 * 4))
#define ELL_EMPTY 0xFFFFu

int psignn_tiles_build(psignn_plan* p, const float* d_pos, int tile_target, hipStream_t st);
void psignn_tiles_free(psignn_plan* p);

// ---------------------------------------------------------------------------------------------
// Optional per-kernel timing with HIP events on the launch stream (bench.py's roofline numbers).
// Off by default: LAUNCH() is then a plain launch.
// ---------------------------------------------------------------------------------------------
extern int g_prof_on;
// the NEXT profiled launch's ALGORITHMIC bytes (every operand read once, every result written once: DESIGN section 4), stated at the
// launch site from what is actually launched (stored pairs swept, kept window, meshes of the shard) -- bench.py builds its roofline
// numbers from these records, not from a re-derivation of the solver's schedule.  Consumed (and reset to 0) by prof_begin.
extern int64_t g_prof_next_bytes;
#define PROF_BYTES(b)                           \
  do {                                          \
    if (g_prof_on) g_prof_next_bytes = (int64_t)(b); \
  } while (0)
void prof_begin(const char* name, hipStream_t st);
void prof_end(hipStream_t st);
#define LAUNCH(name, st, ...)            \
  do {                                   \
    if (g_prof_on) prof_begin(name, st); \
    __VA_ARGS__;                         \
    if (g_prof_on) prof_end(st);         \
  } while (0)

#define FLAG_DIRICHLET 1
#define FLAG_NEUMANN 2

// ---------------------------------------------------------------------------------------------
// Batched Broyden (solver.hip psignn_broyden_solve_batch): one descriptor per mesh of a shard, in device memory.  Every
// per-iteration kernel is launched ONCE for the whole shard with blockIdx.z = mesh; a block loads its mesh's descriptor
// and then runs exactly the code (same block -> element mapping, same partial-sum shapes) of the single-mesh kernels, so
// each mesh's result is bit-identical to its own solve.
// ---------------------------------------------------------------------------------------------
struct BatchDesc {
  int64_t M, ld;
  int32_t nblk, npart, nblk_ax, jgroups, thr, seq_len, keep_trace, n_tiles, tile_base;
  int32_t* st;                 // the mesh's Status block, int32 view
  float *U, *V, *xbuf, *g0, *g1, *upd, *part, *coef, *nrm_part, *jpart;
  double *rel_trace, *abs_trace;
  const struct TileCtx* ctx;
  const float *h0p, *prbp;
  float* part2;                // three-sweep update: block partials of vT.dg, vT.g
  int32_t nblk_u, npart_u;     // its blocks / per-wave partials per stored pair
  float* parta;                // folded sweep 3: per-wave partials of the next iteration's a, contiguous per stored pair
  int32_t nblk4, pad_;         // its blocks (4 floats per lane)
  const float* nrmp;           // mixed family: unit normals in plan order (NULL for dirichlet plans)
  int64_t pstride;             // plane stride of the dot partials (solver.hip: part = 3 planes of (blocks, ldp))
  // batched adjoint solve (psignn_broyden_solve_adjoint_lin_batch): the map's value, the permuted right-hand side, the copy of the
  // iterate the product reads, and the entries of nrm_part the stop test sums (forward: one pair per tile; adjoint: one per block of
  // the unfused residual)
  float *fx, *xcopy;
  const float* grad;
  int32_t n_nrm, pad2_;
};

// Batched transposed product of stored linearisations (fgnn_tile_lin.hip k_vjp_lin_batch): one descriptor per mesh of a shard
struct LinBatchDesc {
  const struct TileCtx* ctx;
  const uint32_t *slot, *tslot;   // the handle's slot dwords and their transposed form
  const float* rec;               // its node records
  const int32_t* vlist;           // mixed handle (Neumann rows stored): its tile list; NULL for a dirichlet handle
  const float* w;                 // out = J^T w, plan order
  float* out;
  const int32_t* st;              // the mesh's Status block, int32 view (done flag)
  int32_t n_slots, slot_base;     // the mesh's entries of the shard's slot list / its first entry
};

// Batched restarted GMRES for the adjoint system (krylov.hip psignn_gmres_solve_adjoint_lin_batch): one descriptor per replica of a
// shard.  Every kernel of the solve is launched ONCE for the shard with blockIdx.z = replica; a block loads its replica's descriptor
// and then runs the single-handle kernel's body, so each replica has the bits of its own solve.
struct GmresBatchDesc {
  int64_t M, ld;
  int32_t nblk, ldp, m, cap;   // cap: entries of each trace
  float *V, *part, *coef;      // the handle's basis, dot partials, coefficients
  double *H, *cs, *sn, *g, *hcol, *y, *res_hist;
  struct GmresState* st;       // cycle state
  struct AdjState* ast;        // solve state
  float *yv, *fy, *ybest;      // the replica's iterate, J^T y, best iterate (its workspace, plan order)
  const float* grad;           // permuted right-hand side
  double *rel_trace, *abs_trace;
};

// Batched Picard / Anderson (fpiter.hip psignn_anderson_solve_batch / psignn_picard_solve_batch): one descriptor per mesh of a shard.
// Every kernel of the iteration is launched ONCE for the shard with blockIdx.z = mesh and runs the single-handle kernel's body on the
// mesh's descriptor; the map is one plain tile launch over the shard's slot list (fgnn_tile.hip k_f_tile_plain_batch), which reads ring
// row X[row] or F[row] of the mesh and writes its scratch row fx.  Each mesh has the bits of its own stepwise solve.
struct FpBatchDesc {
  int64_t M, ld;
  int32_t nblk, npart, n_tiles, tile_base;
  float *X, *F, *low, *part;   // the handle's ring slots, lowest iterate, partials
  float* fx;                   // the map's value at the current trial point (plan order)
  struct FpStatus* st;         // the mesh's status block
  const int32_t* st32;         // ... and its int32 view (done flag of the tile launch)
  double *rel_trace, *abs_trace;
  int32_t* low_idx;
  const struct TileCtx* ctx;
  const float *h0p, *prbp, *nrmp;   // plan-order inputs of the map (nrmp: NULL for dirichlet plans)
};
