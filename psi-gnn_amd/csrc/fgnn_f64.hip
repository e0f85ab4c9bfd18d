// f_theta and the encoder / decoder MLP in float64 (gfx950): the device's own statement of the float64 fixed point, at any size.
//
// replaces: Function.forward run in double precision -- what the reference's --precision switch selects
//           (dirichlet/psignn/utilities/utils.py:28, handed to the reader in dirichlet/psignn/main.py:59-67):
//           dirichlet/psignn/model.py:279-300, mixed/psignn/model.py:216-245, Phi_to / Phi_from / Phi_neumann
//           (model.py:334-368), MLP (model.py:316-332), Encoder / Decoder (model.py:370-392).
//
// This file is the check on the fp32 kernels, so it shares nothing with them but the plan's edge lists:
//   * the arithmetic is written the way the reference writes it: per edge the whole message MLP([x_i | x_j | a_e]) -- first layer on the
//     concatenated 23 inputs, ReLU, second layer with its bias -- and the messages summed per node; nothing is projected once per node,
//     nothing is folded through the second layer, no transposed or packed weight block is read;
//   * the weights are a flat float64 buffer in state-dict order (W64, f64_common.h), not WLayout;
//   * gather form, one node per lane, in the CALLER's numbering: Phi_to sums over the node's in-edges (the plan's CSC), Phi_from and
//     Phi_neumann over its out-edges (CSR), both without self loops and in the plan's canonical order (ascending edge id within a
//     node) -- tiled and untiled plans alike, any degree, duplicate and one-directional edges;
//   * no atomics: every sum has a fixed order, so the same call gives the same bits.
// The handle (psignn_f64, f64_common.h) keeps its own float64 copy of edge_attr in the order of those two lists.
#include "f64_common.h"
#include <math.h>

__global__ void k_f64_attr(int64_t Ep, const int32_t* __restrict__ eid, const void* __restrict__ attr, int is_f64,
                           double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= Ep) return;
  const int64_t e = eid[i];
#pragma unroll
  for (int c = 0; c < 3; ++c)
    out[3 * i + c] = is_f64 ? ((const double*)attr)[3 * e + c] : (double)((const float*)attr)[3 * e + c];   // float32 widens exactly
}

// One message: MLP([x_i | x_j | a]) = W2 relu(W1 [x_i; x_j; a] + b1) + b2, added to acc.
__device__ __forceinline__ void f64_message(const double* __restrict__ Wp, const double* xi, const double* xj, const double* a,
                                            double* acc) {
  using L = W64<2>;   // the Phi block has the same shape in both families
  double z[D];
#pragma unroll
  for (int o = 0; o < D; ++o) {
    const double* w = Wp + L::PHI_W1 + o * L::EIN;
    double s = Wp[L::PHI_B1 + o];
#pragma unroll
    for (int k = 0; k < D; ++k) s = fma(w[k], xi[k], s);
#pragma unroll
    for (int k = 0; k < D; ++k) s = fma(w[D + k], xj[k], s);
#pragma unroll
    for (int k = 0; k < 3; ++k) s = fma(w[2 * D + k], a[k], s);
    z[o] = fmax(s, 0.0);
  }
#pragma unroll
  for (int o = 0; o < D; ++o) {
    const double* w = Wp + L::PHI_W2 + o * D;
    double s = Wp[L::PHI_B2 + o];
#pragma unroll
    for (int k = 0; k < D; ++k) s = fma(w[k], z[k], s);
    acc[o] += s;
  }
}

// sum of the messages of one Phi module over one edge list of node n
__device__ __forceinline__ void f64_phi(const double* __restrict__ Wp, const double* x, const double* __restrict__ h, int32_t beg,
                                        int32_t end, const int32_t* __restrict__ nbr, const double* __restrict__ attr, double* mp) {
#pragma unroll
  for (int o = 0; o < D; ++o) mp[o] = 0.0;
  for (int32_t i = beg; i < end; ++i) {
    const int64_t u = nbr[i];
    double xj[D], a[3];
#pragma unroll
    for (int k = 0; k < D; ++k) xj[k] = h[u * D + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) a[k] = attr[3 * (int64_t)i + k];
    f64_message(Wp, x, xj, a, mp);
  }
}

// One layer, one node per lane.  lofs: the layer's block; nofs: phi_neumann's (mixed).  done: the solver's flag (NULL: none) --
// a launch queued past the solver's last iteration returns at once.
template <int P, bool MIXED>
__global__ __launch_bounds__(256) void k_f64_layer(int64_t N, const double* __restrict__ W, int lofs, int nofs, int apply_ln,
                                                   const int32_t* __restrict__ csr_ptr, const int32_t* __restrict__ csr_nbr,
                                                   const double* __restrict__ csr_attr, const int32_t* __restrict__ csc_ptr,
                                                   const int32_t* __restrict__ csc_nbr, const double* __restrict__ csc_attr,
                                                   const uint8_t* __restrict__ flags, const double* __restrict__ h,
                                                   const double* __restrict__ h0, const double* __restrict__ prb,
                                                   const double* __restrict__ nrm, double* __restrict__ out,
                                                   const int32_t* __restrict__ done) {
  using L = W64<P>;
  if (done && *done) return;
  const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  const uint8_t fl = flags[n];
  if (fl & FLAG_DIRICHLET) {   // Dirichlet rows <- h_initial rows, last of all (model.py:298; mixed/psignn/model.py:243)
#pragma unroll
    for (int o = 0; o < D; ++o) out[n * D + o] = h0[n * D + o];
    return;
  }
  double x[D], y[D];
#pragma unroll
  for (int o = 0; o < D; ++o) x[o] = h[n * D + o];
  const int32_t rb = csr_ptr[n], re = csr_ptr[n + 1];
  if (MIXED && (fl & FLAG_NEUMANN)) {
    // the row is REPLACED by update_neumann([h | Phi_neumann | prb | normal]) (mixed/psignn/model.py:236,241); Phi_neumann has
    // Phi_from's flow: summed at the row index over the out-edges
    double mp[D], cat[L::NCAT], hid[D];
    f64_phi(W + nofs, x, h, rb, re, csr_nbr, csr_attr, mp);
#pragma unroll
    for (int k = 0; k < D; ++k) {
      cat[k] = x[k];
      cat[D + k] = mp[k];
    }
#pragma unroll
    for (int k = 0; k < P; ++k) cat[2 * D + k] = prb[n * P + k];
    cat[2 * D + P] = nrm[2 * n];
    cat[2 * D + P + 1] = nrm[2 * n + 1];
    const double* Wn = W + nofs + L::PHI_SZ;
#pragma unroll
    for (int o = 0; o < D; ++o) {
      double s = Wn[L::NEU_B1 + o];
#pragma unroll
      for (int k = 0; k < L::NCAT; ++k) s = fma(Wn[o * L::NCAT + k], cat[k], s);
      hid[o] = fmax(s, 0.0);
    }
#pragma unroll
    for (int o = 0; o < D; ++o) {
      double s = Wn[L::NEU_B2 + o];
#pragma unroll
      for (int k = 0; k < D; ++k) s = fma(Wn[L::NEU_W2 + o * D + k], hid[k], s);
      y[o] = s;
    }
  } else {
    // cat = [h | Phi_to | Phi_from | prb]; h + sigmoid(alpha(cat)) * update(cat)
    double cat[L::CAT], hid[D];
#pragma unroll
    for (int k = 0; k < D; ++k) cat[k] = x[k];
    f64_phi(W + lofs, x, h, csc_ptr[n], csc_ptr[n + 1], csc_nbr, csc_attr, cat + D);                  // Phi_to: in-edges, summed at the column index
    f64_phi(W + lofs + L::PHI_SZ, x, h, rb, re, csr_nbr, csr_attr, cat + 2 * D);                      // Phi_from: out-edges, summed at the row index
#pragma unroll
    for (int k = 0; k < P; ++k) cat[3 * D + k] = prb[n * P + k];
    double al = W[L::AL_B];
#pragma unroll
    for (int k = 0; k < L::CAT; ++k) al = fma(W[L::AL_W + k], cat[k], al);
    al = 1.0 / (1.0 + exp(-al));
    const double* Wu = W + lofs + 2 * L::PHI_SZ;
#pragma unroll
    for (int o = 0; o < D; ++o) {
      double s = Wu[L::UPD_B1 + o];
#pragma unroll
      for (int k = 0; k < L::CAT; ++k) s = fma(Wu[o * L::CAT + k], cat[k], s);
      hid[o] = fmax(s, 0.0);
    }
#pragma unroll
    for (int o = 0; o < D; ++o) {
      double s = Wu[L::UPD_B2 + o];
#pragma unroll
      for (int k = 0; k < D; ++k) s = fma(Wu[L::UPD_W2 + o * D + k], hid[k], s);
      y[o] = x[o] + al * s;
    }
  }
  if (apply_ln) {   // LayerNorm(10), eps 1e-5, biased variance, affine (model.py:293)
    double mu = 0.0;
#pragma unroll
    for (int o = 0; o < D; ++o) mu += y[o];
    mu /= D;
    double var = 0.0;
#pragma unroll
    for (int o = 0; o < D; ++o) var = fma(y[o] - mu, y[o] - mu, var);
    var /= D;
    const double rs = 1.0 / sqrt(var + 1e-5);
#pragma unroll
    for (int o = 0; o < D; ++o) y[o] = (y[o] - mu) * rs * W[L::LN_G + o] + W[L::LN_B + o];
  }
#pragma unroll
  for (int o = 0; o < D; ++o) out[n * D + o] = y[o];
}

// out (n, dout) = W2 relu(W1 x + b1) + b2, one row per lane; din, hid, dout <= 16
__global__ __launch_bounds__(256) void k_mlp2_f64(const double* __restrict__ x, int64_t n, int din, int hid, int dout,
                                                  const double* __restrict__ w1, const double* __restrict__ b1,
                                                  const double* __restrict__ w2, const double* __restrict__ b2,
                                                  double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double xi[16], z[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) xi[k] = k < din ? x[i * din + k] : 0.0;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    double s = 0.0;
    if (j < hid) {
      s = b1[j];
#pragma unroll
      for (int k = 0; k < 16; ++k)
        if (k < din) s = fma(w1[j * din + k], xi[k], s);
    }
    z[j] = fmax(s, 0.0);
  }
  for (int o = 0; o < dout; ++o) {
    double s = b2[o];
#pragma unroll
    for (int j = 0; j < 16; ++j)
      if (j < hid) s = fma(w2[o * hid + j], z[j], s);
    out[i * dout + o] = s;
  }
}

// ---------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------
extern "C" int64_t psignn_f64_weights_size(int mixed, int n_layers) {
  if (n_layers < 1) return -1;
  return mixed ? W64<3>::total(n_layers, true) : W64<2>::total(n_layers, false);
}

extern "C" void psignn_f64_destroy(psignn_f64_t* f) {
  if (!f) return;
  void* ptrs[] = {f->csr_attr, f->csc_attr, f->pp[0], f->pp[1]};
  for (void* q : ptrs)
    if (q) (void)hipFree(q);
  delete f;
}

extern "C" int psignn_f64_create(psignn_f64_t** out, const psignn_plan_t* p, const void* d_edge_attr, int attr_is_f64, void* stream) {
  ARG_CHECK(out != nullptr, "out is NULL");
  *out = nullptr;
  ARG_CHECK(p != nullptr && d_edge_attr != nullptr, "NULL argument");
  ARG_CHECK(attr_is_f64 == 0 || attr_is_f64 == 1, "attr_is_f64 must be 0 or 1");
  hipStream_t st = (hipStream_t)stream;
  psignn_f64* f = new psignn_f64();
  f->p = p;
  const int64_t Ep = p->Ep;
  const size_t bytes = (size_t)(Ep > 0 ? Ep : 1) * 3 * sizeof(double);
  hipError_t e = hipMalloc((void**)&f->csr_attr, bytes);
  if (e == hipSuccess) e = hipMalloc((void**)&f->csc_attr, bytes);
  if (e == hipSuccess && Ep > 0) {
    const unsigned g = (unsigned)cdiv(Ep, 256);
    k_f64_attr<<<g, 256, 0, st>>>(Ep, p->csr_eid, d_edge_attr, attr_is_f64, f->csr_attr);
    k_f64_attr<<<g, 256, 0, st>>>(Ep, p->csc_eid, d_edge_attr, attr_is_f64, f->csc_attr);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(st);   // d_edge_attr may go when create returns
  }
  if (e != hipSuccess) {
    psignn_set_error("psignn_f64_create: %s (two float64 copies of edge_attr, %zu bytes each)", hipGetErrorString(e), bytes);
    psignn_f64_destroy(f);
    return PSIGNN_EHIP;
  }
  *out = f;
  return PSIGNN_OK;
}

const psignn_plan* psignn_f64_plan(const psignn_f64_t* f) { return f ? f->p : nullptr; }

template <int P, bool MIXED>
static void f64_launch(const psignn_f64* f, const double* W, int nl, int l, int apply_ln, const double* h, const double* h0,
                       const double* prb, const double* nrm, double* out, const int32_t* done, hipStream_t st) {
  using L = W64<P>;
  const psignn_plan* p = f->p;
  // algorithmic bytes: both edge lists once (neighbour id, 3 attributes, the neighbour's row), per node its row in and out, prb, pointers
  PROF_BYTES(2 * p->Ep * (4 + 24 + 8 * D) + p->N * (16 * D + 8 * P + 17));
  LAUNCH("k_f64_layer", st,
         (k_f64_layer<P, MIXED><<<(unsigned)cdiv(p->N, 256), 256, 0, st>>>(
             p->N, W, L::layer(l), L::layer(nl), apply_ln, F64_EDGES(f), h, h0, prb, nrm, out, done)));
}

// f in the caller's numbering; done: see k_f64_layer
int psignn_f64_eval(psignn_f64_t* f, const double* W, int nl, const double* h, const double* h0, const double* prb, const double* nrm,
                    double* out, const int32_t* done, hipStream_t st) {
  ARG_CHECK(f && W && h && h0 && prb && out, "NULL argument");
  ARG_CHECK(nl >= 1 && nl <= 64, "n_layers out of range");
  ARG_CHECK(!f->p->mixed || nrm, "mixed plan needs unit normals");
  ARG_CHECK(out != h, "out must not alias h");
  if (f->p->N == 0) return PSIGNN_OK;
  if (f->p->mixed) {
    // The reference's mixed loop never reassigns h: every layer reads the ORIGINAL h and only the last layer's h_next is returned
    // (mixed/psignn/model.py:221-245) -- so the last layer on h IS the block.
    f64_launch<3, true>(f, W, nl, nl - 1, 1, h, h0, prb, nrm, out, done, st);
  } else {
    if (nl > 1 && !f->pp[0]) {
      const size_t bytes = (size_t)f->p->N * D * sizeof(double);
      for (int i = 0; i < 2; ++i)
        if (hipMalloc((void**)&f->pp[i], bytes) != hipSuccess) {
          f->pp[i] = nullptr;
          if (i == 1) { (void)hipFree(f->pp[0]); f->pp[0] = nullptr; }
          psignn_set_error("psignn_f64_forward: no memory for the layer states (2 x %zu bytes)", bytes);
          return PSIGNN_ENOMEM;
        }
    }
    const double* cur = h;
    for (int l = 0; l < nl; ++l) {
      double* dst = l == nl - 1 ? out : f->pp[l & 1];
      f64_launch<2, false>(f, W, nl, l, l == nl - 1, cur, h0, prb, nrm, dst, done, st);
      cur = dst;
    }
  }
  HIP_TRY(hipGetLastError());
  return PSIGNN_OK;
}

extern "C" int psignn_f64_forward(psignn_f64_t* f, const double* W, int nl, const double* h, const double* h0, const double* prb,
                                  const double* nrm, double* out, void* stream) {
  return psignn_f64_eval(f, W, nl, h, h0, prb, nrm, out, nullptr, (hipStream_t)stream);
}

extern "C" int psignn_mlp2_f64(const double* x, int64_t n, int din, int hid, int dout, const double* w1, const double* b1,
                               const double* w2, const double* b2, double* out, void* stream) {
  ARG_CHECK(x && w1 && b1 && w2 && b2 && out, "NULL argument");
  ARG_CHECK(n >= 0 && din >= 1 && din <= 16 && hid >= 1 && hid <= 16 && dout >= 1 && dout <= 16, "bad sizes");
  if (n == 0) return PSIGNN_OK;
  k_mlp2_f64<<<(unsigned)cdiv(n, 256), 256, 0, (hipStream_t)stream>>>(x, n, din, hid, dout, w1, b1, w2, b2, out);
  HIP_TRY(hipGetLastError());
  return PSIGNN_OK;
}
