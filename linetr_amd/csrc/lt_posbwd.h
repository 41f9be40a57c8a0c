// The two positional encoders and the token assembly of KeylineEncoder for TRAINING with a backward (models/line_transformer.py:40-73 and
// :113-121 of the reference).  Every layer of the encoders but the first is a GEMM with a native backward already (lt_linbwd.h, lt_bnbwd.h);
// what has no kernel beside them is here: two kernel pairs on float32 rows, bound by bytes.
//
//   The encoders' input layer, Conv1d(Kin -> N, k = 1) with Kin = 5 (lines) or 3 (words), no GEMM:
//     z [rows][N of ldz] = x [rows][Kin of ldx] W^T + b        W [N][Kin], 1 <= Kin <= 8, N % 4 == 0, 4 <= N <= 64
//     dW [N][Kin] = g^T x        db [N] = sum_r g        (g [rows][N of ldg]: the dz the BatchNorm backward hands down; no mask, no dx)
//   il_fwd_kernel: the weights and the bias in LDS (at most 576 floats), a thread owns four channels of a row: Kin scalar loads of the
//   narrow row (any alignment; the N / 4 threads of a row read the same words), one fmaf chain per channel in ascending k starting at the
//   bias, one 16-byte store.  il_bwd_partial_kernel: a block owns IL_CHUNK rows; thread (phase p, quad q) walks rows p, p + P, .. of the
//   chunk (P = 256 / (N / 4) phases) with 4 (Kin + 1) accumulators, the phases are added in ascending order through LDS and the block
//   writes one partial [Kin + 1][N] (row k: column k of dW; row Kin: db).  il_bwd_reduce_kernel adds the chunks in float64 in one fixed
//   ascending order (ordered_column_sum: sixteen contiguous ranges of chunks, one per wave, then the ranges in order).
//
//   The token assembly, per segment (sub-line) l of S tokens:  x [L][S + 1][256],  x[l][0] = cls,  x[l][1 + t] = desc[l][t] + pos[l][t]
//   (one float32 add);  backward from dx [L][S + 1][256] in one pass:  dtok [L S][256] = dx[:, 1:] as contiguous rows (the gradient of
//   desc and of pos alike),  dcls [256] = sum_l dx[l][0].
//   ta_fwd_kernel: one wave per output row, lane i owns columns 4 i .. 4 i + 3.  ta_bwd_kernel: a block owns TA_SEGS segments, wave w the
//   segments w, w + 4, .. of them: it copies their token rows (TA_ROWS rows in flight) and adds their CLS rows in segment order; the four
//   waves' sums are added in wave order into one partial row per block.  ta_reduce_kernel adds the partial rows in float64 by the same
//   ordered_column_sum (the scheme of ln_reduce_kernel, lt_descbwd.h, with sixteen loads' latencies side by side instead of one).
//
// Deterministic: no atomics, every sum in a fixed order.  Every output element is written; nothing at or beyond the last row, or beyond a
// row's width, is loaded or stored.
#pragma once
#include "lt_common.h"

namespace lt {

constexpr int IL_MAX_K = 8;        // input channels of the input layer, at most
constexpr int IL_MAX_N = 64;       // output channels, at most
constexpr int IL_CHUNK = 256;      // rows of one chunk of the input layer's weight-gradient reduction
constexpr int TA_SEGS = 8;         // segments per block of ta_bwd_kernel = per partial row of dcls
constexpr int TA_ROWS = 8;         // token rows in flight per wave of ta_bwd_kernel
constexpr int TA_MAX_S = 255;      // tokens per segment: the CLS slot takes the 256th row cls_token_pool accepts

// grid ceil(rows (N / 4) / 256), 256 threads.  b may be null (no bias).
__global__ __launch_bounds__(256) void il_fwd_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ W,
                                                     const float* __restrict__ b, int64_t rows, int N, int Kin, float* __restrict__ z,
                                                     int64_t ldz) {
  __shared__ float Ws[IL_MAX_N * IL_MAX_K];
  __shared__ __attribute__((aligned(16))) float bs[IL_MAX_N];
  for (int i = threadIdx.x; i < N * Kin; i += 256) Ws[i] = W[i];
  if (threadIdx.x < N) bs[threadIdx.x] = b ? b[threadIdx.x] : 0.f;
  __syncthreads();
  const int nq = N / 4;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * nq) return;
  const int64_t row = i / nq;
  const int c = (int)(i - row * nq) * 4;
  const float* xr = x + row * ldx;
  float xv[IL_MAX_K];
#pragma unroll
  for (int k = 0; k < IL_MAX_K; ++k) xv[k] = k < Kin ? xr[k] : 0.f;
  f32x4 acc = *reinterpret_cast<const f32x4*>(bs + c);
#pragma unroll
  for (int k = 0; k < IL_MAX_K; ++k) {
    if (k < Kin) {
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] = fmaf(xv[k], Ws[(c + e) * Kin + k], acc[e]);
    }
  }
  *reinterpret_cast<f32x4*>(z + row * ldz + c) = acc;
}

// grid cdiv(rows, IL_CHUNK), 256 threads.  partial [gridDim.x][Kin + 1][N]
__global__ __launch_bounds__(256) void il_bwd_partial_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ g,
                                                             int64_t ldg, int64_t rows, int N, int Kin, float* __restrict__ partial) {
  __shared__ float red[(IL_MAX_K + 1) * 4][256];       // [accumulator][thread]: conflict-free both ways
  const int nq = N / 4, phases = 256 / nq;
  const int p = threadIdx.x / nq, q = threadIdx.x - p * nq;
  const int64_t r0 = (int64_t)blockIdx.x * IL_CHUNK;
  const int64_t r1 = r0 + IL_CHUNK < rows ? r0 + IL_CHUNK : rows;
  f32x4 acc[IL_MAX_K + 1];
#pragma unroll
  for (int k = 0; k <= IL_MAX_K; ++k) acc[k] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (p < phases) {
    for (int64_t row = r0 + p; row < r1; row += phases) {
      const f32x4 gv = *reinterpret_cast<const f32x4*>(g + row * ldg + q * 4);
      const float* xr = x + row * ldx;
#pragma unroll
      for (int k = 0; k < IL_MAX_K; ++k) {
        if (k < Kin) {
          const float xv = xr[k];
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[k][e] = fmaf(gv[e], xv, acc[k][e]);
        }
      }
      acc[IL_MAX_K] += gv;
    }
  }
#pragma unroll
  for (int k = 0; k <= IL_MAX_K; ++k) {
    if (k < Kin || k == IL_MAX_K) {
      const int a = (k == IL_MAX_K ? Kin : k) * 4;
#pragma unroll
      for (int e = 0; e < 4; ++e) red[a + e][threadIdx.x] = acc[k][e];
    }
  }
  __syncthreads();
  // output o = (accumulator a = 4 k + e, quad q'): the phases in ascending order
  float* out = partial + (int64_t)blockIdx.x * (Kin + 1) * N;
  for (int o = threadIdx.x; o < (Kin + 1) * N; o += 256) {
    const int a = o / nq, qq = o - a * nq;
    float s = red[a][qq];
    for (int ph = 1; ph < phases; ++ph) s += red[a][ph * nq + qq];
    out[(a >> 2) * N + qq * 4 + (a & 3)] = s;
  }
}

// The ordered sum both reduce kernels share: column i of `rows` partial rows of `stride` floats, in float64.  The RED_WAVES waves of a
// block own contiguous ranges of the rows in ascending order (a lane owns a column: a row is one coalesced load of a wave; RED_LOADS
// loads in flight, added in row order), and wave 0 adds the waves' sums in wave order: one fixed order, whatever the grid.
constexpr int RED_WAVES = 16;
constexpr int RED_LOADS = 8;
__device__ __forceinline__ double ordered_column_sum(const float* __restrict__ partial, int rows, int64_t stride, int i, bool live,
                                                     double (*red)[64]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int per = (rows + RED_WAVES - 1) / RED_WAVES;
  const int r0 = wave * per, r1 = r0 + per < rows ? r0 + per : rows;
  double s = 0.0;
  if (live) {
    for (int r = r0; r < r1; r += RED_LOADS) {
      float v[RED_LOADS];
#pragma unroll
      for (int j = 0; j < RED_LOADS; ++j) v[j] = r + j < r1 ? partial[(int64_t)(r + j) * stride + i] : 0.f;
#pragma unroll
      for (int j = 0; j < RED_LOADS; ++j) s += (double)v[j];
    }
  }
  red[wave][lane] = s;
  __syncthreads();
  if (wave == 0) {
    s = red[0][lane];
#pragma unroll
    for (int w = 1; w < RED_WAVES; ++w) s += red[w][lane];
  }
  return s;       // (wave 0 holds the sum)
}

// grid cdiv((Kin + 1) N, 64), 1024 threads: lane i of a block owns element blockIdx.x * 64 + i of the partials.  dW / db may be null.
__global__ __launch_bounds__(1024) void il_bwd_reduce_kernel(const float* __restrict__ partial, int chunks, int N, int Kin,
                                                             float* __restrict__ dW, float* __restrict__ db) {
  __shared__ double red[RED_WAVES][64];
  const int i = blockIdx.x * 64 + (threadIdx.x & 63);
  const int total = (Kin + 1) * N;
  const double s = ordered_column_sum(partial, chunks, total, i, i < total, red);
  if (threadIdx.x >= 64 || i >= total) return;
  const int k = i / N, n = i - k * N;
  if (k < Kin) { if (dW) dW[n * Kin + k] = (float)s; }
  else if (db) db[n] = (float)s;
}

// ---- the token assembly ------------------------------------------------------------------------------------------------------------

// grid ceil(L (S + 1) / 4), 256 threads: one wave per row of x [L][S + 1][256].  desc, pos [L S][256]; cls [256]
__global__ __launch_bounds__(256) void ta_fwd_kernel(const float* __restrict__ desc, const float* __restrict__ pos,
                                                     const float* __restrict__ cls, int64_t L, int S, float* __restrict__ x) {
  const int c = (threadIdx.x & 63) * 4;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= L * (S + 1)) return;
  const int64_t l = row / (S + 1);
  const int t = (int)(row - l * (S + 1));
  f32x4 v;
  if (t == 0) {
    v = *reinterpret_cast<const f32x4*>(cls + c);
  } else {
    const int64_t src = (l * S + (t - 1)) * D + c;
    v = *reinterpret_cast<const f32x4*>(desc + src) + *reinterpret_cast<const f32x4*>(pos + src);
  }
  *reinterpret_cast<f32x4*>(x + row * D + c) = v;
}

// grid ceil(L / TA_SEGS), 256 threads.  dx [L][S + 1][256] -> dtok [L S][256] (null: not wanted), partial [gridDim.x][256] (null: not
// wanted): the sum of the block's CLS rows
__global__ __launch_bounds__(256) void ta_bwd_kernel(const float* __restrict__ dx, int64_t L, int S, float* __restrict__ dtok,
                                                     float* __restrict__ partial) {
  __shared__ f32x4 red[3][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = lane * 4;
  const int64_t l0 = (int64_t)blockIdx.x * TA_SEGS;
  const int64_t l1 = l0 + TA_SEGS < L ? l0 + TA_SEGS : L;
  f32x4 sum = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int64_t l = l0 + wave; l < l1; l += 4) {
    const float* src = dx + l * (S + 1) * D + c;
    if (partial) sum += *reinterpret_cast<const f32x4*>(src);
    if (dtok) {
      float* dst = dtok + l * S * D + c;
      for (int t0 = 0; t0 < S; t0 += TA_ROWS) {
        f32x4 v[TA_ROWS];
#pragma unroll
        for (int j = 0; j < TA_ROWS; ++j)
          if (t0 + j < S) v[j] = *reinterpret_cast<const f32x4*>(src + (int64_t)(t0 + j + 1) * D);
#pragma unroll
        for (int j = 0; j < TA_ROWS; ++j)
          if (t0 + j < S) *reinterpret_cast<f32x4*>(dst + (int64_t)(t0 + j) * D) = v[j];
      }
    }
  }
  if (!partial) return;
  if (wave > 0) red[wave - 1][lane] = sum;
  __syncthreads();
  if (wave == 0) {
#pragma unroll
    for (int w = 0; w < 3; ++w) sum += red[w][lane];       // wave order
    *reinterpret_cast<f32x4*>(partial + (int64_t)blockIdx.x * D + c) = sum;
  }
}

// grid 4, 1024 threads: lane i of a block owns column blockIdx.x * 64 + i of the partial rows
__global__ __launch_bounds__(1024) void ta_reduce_kernel(const float* __restrict__ partial, int blocks, float* __restrict__ dcls) {
  __shared__ double red[RED_WAVES][64];
  const int i = blockIdx.x * 64 + (threadIdx.x & 63);
  const double s = ordered_column_sum(partial, blocks, D, i, true, red);
  if (threadIdx.x < 64) dcls[i] = (float)s;
}

}  // namespace lt
