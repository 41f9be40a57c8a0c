// BatchNorm1d (+ optional ReLU) for TRAINING with a backward, SURVEY.md section 8(f) row 4: the link of the signature layer's MLP
// (Conv1d(512, 512) -> BatchNorm1d(512) -> ReLU -> Conv1d(512, 256), models/line_transformer.py:157-166) that lt_linbwd.h and
// lt_attnbwd.h leave open.  z [rows][C] with a row stride, the widths and strides of bn_train_layer (lt_bntrain.h).
//
// The forward is lt_bntrain.h's (bn_forward_launch), out of place -- z is kept: the backward reads it -- and with the saved statistics
// float64 [mean[C] | invstd[C]].  Here is the backward, as torch autograd differentiates relu(batch_norm(z)):  g' = g where y > 0
// else 0 (y: the layer's own output, nothing is recomputed to decide a sign; no y: g' = g),  xhat = (z - mean) invstd,
//   dbeta = sum_r g'      dgamma = sum_r g' xhat      dz = gamma invstd (g' - dbeta / n - xhat dgamma / n)       (eval: dz = gamma invstd g')
//   bn_bwd_partial_kernel   per row chunk (the forward's chunking) and channel: sum g' and sum g' (z - mean), float64, z - mean formed
//                           against the float64 mean; one partial row per block, no atomics
//   bn_bwd_finalize_kernel  chunks added in block order; dbeta, dgamma = invstd sum g' (z - mean) as float32; the apply step's
//                           coefficients k1 = fl(gamma invstd), k2 = fl(k1 dbeta / n), k3 = fl(k1 invstd^2 sum g' (z - mean) / n) as float32
//                           (k2 and k3 from the ROUNDED k1: with one row k1 g' - k2 is exactly 0); eval: k2 = k3 = 0
//   bn_bwd_apply_kernel     dz = k1 g' - k2 - k3 fl((double)z - mean): float32, no contraction, four channels per thread
// HBM-bound: g, y and z are read twice, dz written once.  Every access of a row is 16 bytes per lane.  Deterministic: fixed summation order.
#pragma once
#include "lt_bntrain.h"

namespace lt {

constexpr int BNB_QUADS = 32;      // channel quads side by side in a block of bn_bwd_partial_kernel (128 channels, 512 bytes of a row)
constexpr int BNB_RP = 8;          // rows in parallel

// grid (row chunks, ceil(C / 4 / BNB_QUADS)); partial [gridDim.x][2 C]: sum g' | sum g' (z - mean).  A block whose chunk lies behind
// the last row writes zero partials.  y may be null (no mask).
__global__ __launch_bounds__(256) void bn_bwd_partial_kernel(const float* __restrict__ g, int64_t ldg, const float* __restrict__ y, int64_t ldy,
                                                             const float* __restrict__ z, int64_t ldz, const double* __restrict__ save,
                                                             int64_t rows, int C, double* __restrict__ partial) {
  __shared__ double red[BNB_RP][BNB_QUADS][8];
  const int tid = threadIdx.x;
  const int q_in = tid % BNB_QUADS, r_in = tid / BNB_QUADS;
  const int c = (blockIdx.y * BNB_QUADS + q_in) * 4;
  const bool owns = c < C;
  const int64_t chunk = (rows + gridDim.x - 1) / gridDim.x;
  const int64_t r0 = (int64_t)blockIdx.x * chunk, r1 = r0 + chunk < rows ? r0 + chunk : rows;
  double s[4] = {0.0, 0.0, 0.0, 0.0}, q[4] = {0.0, 0.0, 0.0, 0.0};
  if (owns) {
    double mean[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) mean[k] = save[c + k];
#pragma unroll 2
    for (int64_t r = r0 + r_in; r < r1; r += BNB_RP) {
      f32x4 gv = *reinterpret_cast<const f32x4*>(g + r * ldg + c);
      const f32x4 zv = *reinterpret_cast<const f32x4*>(z + r * ldz + c);
      if (y) {
        const f32x4 yv = *reinterpret_cast<const f32x4*>(y + r * ldy + c);
#pragma unroll
        for (int k = 0; k < 4; ++k) gv[k] = yv[k] > 0.f ? gv[k] : 0.f;
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const double gd = (double)gv[k];
        s[k] += gd;
        q[k] += gd * ((double)zv[k] - mean[k]);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) { red[r_in][q_in][k] = s[k]; red[r_in][q_in][4 + k] = q[k]; }
  __syncthreads();
  if (owns && r_in == 0) {
    for (int j = 1; j < BNB_RP; ++j)       // fixed order
#pragma unroll
      for (int k = 0; k < 4; ++k) { s[k] += red[j][q_in][k]; q[k] += red[j][q_in][4 + k]; }
    double* out = partial + (int64_t)blockIdx.x * 2 * C;
#pragma unroll
    for (int k = 0; k < 4; ++k) { out[c + k] = s[k]; out[C + c + k] = q[k]; }
  }
}

// one thread per channel; coef [3 C]: k1 | k2 | k3.  dgamma / dbeta may be null.  n_blocks = 0: no sums (eval mode without them).
__global__ __launch_bounds__(256) void bn_bwd_finalize_kernel(const double* __restrict__ partial, int n_blocks, int C, int64_t rows,
                                                              const float* __restrict__ gamma, const double* __restrict__ save, int eval,
                                                              float* __restrict__ dgamma, float* __restrict__ dbeta, float* __restrict__ coef) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  double s = 0.0, q = 0.0;
  for (int b = 0; b < n_blocks; ++b) { s += partial[(int64_t)b * 2 * C + c]; q += partial[(int64_t)b * 2 * C + C + c]; }
  const double invstd = save[C + c];
  if (dbeta) dbeta[c] = (float)s;
  if (dgamma) dgamma[c] = (float)(q * invstd);
  const float k1 = (float)((double)gamma[c] * invstd);
  const double n = (double)rows;
  coef[c] = k1;
  coef[C + c] = eval ? 0.f : (float)((double)k1 * s / n);
  coef[2 * C + c] = eval ? 0.f : (float)((double)k1 * invstd * invstd * q / n);
}

// four channels per thread.  y may be null (no mask); eval: z is not read.
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const float* __restrict__ g, int64_t ldg, const float* __restrict__ y, int64_t ldy,
                                                           const float* __restrict__ z, int64_t ldz, const double* __restrict__ save,
                                                           const float* __restrict__ coef, int64_t rows, int C, int eval,
                                                           float* __restrict__ dz, int64_t lddz) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int c4 = C / 4;
  if (i >= rows * c4) return;
  const int64_t r = i / c4;
  const int c = (int)(i - r * c4) * 4;
  f32x4 gv = *reinterpret_cast<const f32x4*>(g + r * ldg + c);
  if (y) {
    const f32x4 yv = *reinterpret_cast<const f32x4*>(y + r * ldy + c);
#pragma unroll
    for (int k = 0; k < 4; ++k) gv[k] = yv[k] > 0.f ? gv[k] : 0.f;
  }
  const f32x4 k1 = *reinterpret_cast<const f32x4*>(coef + c);
  f32x4 out;
  if (eval) {
#pragma unroll
    for (int k = 0; k < 4; ++k) out[k] = k1[k] * gv[k];
  } else {
    const f32x4 zv = *reinterpret_cast<const f32x4*>(z + r * ldz + c);
    const f32x4 k2 = *reinterpret_cast<const f32x4*>(coef + C + c), k3 = *reinterpret_cast<const f32x4*>(coef + 2 * C + c);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma clang fp contract(off)
      const float d = (float)((double)zv[k] - save[c + k]);
      out[k] = k1[k] * gv[k] - k2[k] - k3[k] * d;
    }
  }
  *reinterpret_cast<f32x4*>(dz + r * lddz + c) = out;
}

}  // namespace lt
