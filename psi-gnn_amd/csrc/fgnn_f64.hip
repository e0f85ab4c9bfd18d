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
// The layer itself -- message sums, gate, update MLP, LayerNorm -- is the node block of f64_node.h without a tangent
// (k_f64_jvp_layer<P, MIXED, false>, in the launch records k_f64_layer), the same statement the float64 derivatives differentiate;
// this file holds the attribute copy, the encoder / decoder MLP and the host side.
#include "f64_common.h"
#include "f64_node.h"
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

// one layer: the plain (TAN = false) layer kernel of f64_node.h
static void f64_launch(const psignn_f64* f, const double* W, int nl, int l, int apply_ln, const double* h, const double* h0,
                       const double* prb, const double* nrm, double* out, const int32_t* done, hipStream_t st) {
  const psignn_plan* p = f->p;
  // algorithmic bytes: both edge lists once (neighbour id, 3 attributes, the neighbour's row), per node its row in and out, prb, pointers
  F64_FAMILY(p->mixed, PROF_BYTES(2 * p->Ep * (4 + 24 + 8 * D) + p->N * (16 * D + 8 * P + 17));
             LAUNCH("k_f64_layer", st,
                    (k_f64_jvp_layer<P, MIXED, false><<<(unsigned)cdiv(p->N, 256), 256, 0, st>>>(
                        p->N, W, L::layer(l), L::layer(nl), apply_ln, F64_EDGES(f), h, nullptr, h0, prb, nrm, out, nullptr, done))));
}

// f in the caller's numbering; done: the flag of a solver, see k_f64_jvp_layer
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
    f64_launch(f, W, nl, nl - 1, 1, h, h0, prb, nrm, out, done, st);
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
      f64_launch(f, W, nl, l, l == nl - 1, cur, h0, prb, nrm, dst, done, st);
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
