// BatchNorm1d in TRAINING mode (batch statistics) for the training-time forward, SURVEY.md section 8(f) row 4:
// the reference's MLP stacks are Conv1d(k=1) + BatchNorm1d + ReLU (models/line_transformer.py:9-20) and train.py:127 puts the
// model in train mode, so every BatchNorm normalises with the mean / biased variance of the CURRENT batch -- over all B * N (* T)
// positions -- and moves its running statistics towards them (momentum 0.1, unbiased variance).  The eval path folds the running
// statistics into the convolution at linetr_create; here the convolution stays unfolded (LinetrModelConfig::bn_batch_stats), its
// pre-activations z [rows][C] are written by the GEMM, and three small kernels do the rest:
//   bn_partial_kernel    per-channel sum / sum of squares of a row chunk, float64 accumulators (torch's CPU kernel accumulates a float
//                        batch in double as well), one partial row per block -- no atomics, so the result is deterministic
//   bn_finalize_kernel   partials combined in block order -> mean, biased var, alpha = gamma / sqrt(var + eps), beta' = beta - mean alpha
//                        (the affine form torch's batch_norm_cpu_transform_input applies), running statistics updated in place;
//                        on request this batch's mean | var as float32 and mean | invstd as float64 (what a backward reads)
//   bn_apply_kernel      y = z alpha + beta', with or without max(., 0); y may be z
// HBM-bound elementwise work (one read for the statistics, one read + write for the transform); coalesced along the channel axis.
// This is the one BatchNorm forward: bn_forward_launch makes the three launches for linetr_forward_train (bn_train_layer: in place,
// ReLU, packed statistics) and for linetr_bn_forward (linetr_train.hip: out of place so that z survives for the backward of
// lt_bnbwd.h, saved statistics, and an eval mode that takes mean | var from the running statistics and launches no bn_partial_kernel).
// Both run the same statements in the same order, so their y, alpha | beta' and running statistics agree bit for bit.
// The kernels have internal linkage: two translation units include this header (linetr_net.hip and linetr_train.hip), each with its
// own copy.
#pragma once
#include "lt_handle.h"

namespace lt {

constexpr int BN_MAX_BLOCKS = 512;     // row chunks of bn_partial_kernel (two per CU)
// (BN_MAX_CHANNELS, lt_common.h: the widest BatchNorm layer the statistics scratch is sized for)

// what a training-time forward hands down to forward_core (linetr_forward_train)
struct BnTrain {
  float* running = nullptr;     // packed [layer][mean[C] | var[C]], updated in place
  float* batch = nullptr;       // packed like `running`: this batch's mean | BIASED variance (may be null)
  float momentum = 0.1f;
  double* partial = nullptr;    // [BN_MAX_BLOCKS][2 * 512] scratch
  float* affine = nullptr;      // [2 * 512] scratch: alpha | beta'
};

// z [rows][C] (row stride ld), any C <= BN_MAX_CHANNELS; partial [gridDim.x][2 C].  A block whose chunk lies behind the last row
// writes zero partials.
static __global__ __launch_bounds__(256) void bn_partial_kernel(const float* __restrict__ z, int64_t rows, int C, int ld,
                                                         double* __restrict__ partial) {
  __shared__ double red[2][256];
  const int tid = threadIdx.x;
  const int cw = C < 256 ? C : 256;            // channels side by side in a block pass
  const int rp = 256 / cw;                     // rows in parallel
  const int r_in = tid / cw, c_in = tid % cw;  // (256 % cw != 0: the threads with r_in == rp own nothing)
  const int64_t chunk = (rows + gridDim.x - 1) / gridDim.x;
  const int64_t r0 = (int64_t)blockIdx.x * chunk, r1 = r0 + chunk < rows ? r0 + chunk : rows;
  // the trip count is the block's, not the thread's (C = 260: lanes 0-3 alone have a second channel), so that every thread reaches
  // the barriers; loads and stores are guarded instead
  for (int c0 = 0; c0 < C; c0 += 256) {
    const int c = c0 + c_in;
    const bool owns = c < C && r_in < rp;
    double s = 0.0, q = 0.0;
    if (owns)
      for (int64_t r = r0 + r_in; r < r1; r += rp) {
        const double v = (double)z[r * ld + c];
        s += v;
        q += v * v;
      }
    red[0][tid] = s;
    red[1][tid] = q;
    __syncthreads();
    if (owns && r_in == 0) {
      for (int k = 1; k < rp; ++k) { s += red[0][k * cw + c_in]; q += red[1][k * cw + c_in]; }   // fixed order
      partial[(int64_t)blockIdx.x * 2 * C + c] = s;
      partial[(int64_t)blockIdx.x * 2 * C + C + c] = q;
    }
    __syncthreads();
  }
}

// one thread per channel.  Every output but affine may be null.  Train mode (eval = 0): mean | var from the partials, and running, if
// present, is updated in place.  Eval mode: mean | var = running, which is only read; partial is not read.
static __global__ __launch_bounds__(256) void bn_finalize_kernel(const double* __restrict__ partial, int n_blocks, int C, int64_t rows,
                                                          const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                          float momentum, float* __restrict__ running /*mean[C] | var[C]*/, int eval,
                                                          float* __restrict__ batch /*mean[C] | biased var[C]*/,
                                                          float* __restrict__ affine /*alpha[C] | beta'[C]*/,
                                                          double* __restrict__ save /*mean[C] | invstd[C]*/) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  const double n = (double)rows;
  double mean, var;
  if (eval) {
    mean = (double)running[c];
    var = (double)running[C + c];
  } else {
    double s = 0.0, q = 0.0;
    for (int b = 0; b < n_blocks; ++b) { s += partial[(int64_t)b * 2 * C + c]; q += partial[(int64_t)b * 2 * C + C + c]; }
    mean = s / n;
    var = q / n - mean * mean;                 // biased (what the normalisation uses)
    if (var < 0.0) var = 0.0;
  }
  const double invstd = 1.0 / sqrt(var + (double)eps);
  const double alpha = (double)gamma[c] * invstd;
  affine[c] = (float)alpha;
  affine[C + c] = (float)((double)beta[c] - mean * alpha);
  if (batch) { batch[c] = (float)mean; batch[C + c] = (float)var; }
  if (save) { save[c] = mean; save[C + c] = invstd; }
  if (!eval && running) {
    // running statistics: (1 - momentum) old + momentum new, the variance unbiased (torch.nn.BatchNorm1d)
    const double unbiased = rows > 1 ? var * n / (n - 1.0) : var;
    running[c] = (float)((1.0 - (double)momentum) * (double)running[c] + (double)momentum * mean);
    running[C + c] = (float)((1.0 - (double)momentum) * (double)running[C + c] + (double)momentum * unbiased);
  }
}

// y = z alpha + beta' (relu: max(., 0)), two roundings; four channels per thread (C % 4 == 0, ldz % 4 == 0, ldy % 4 == 0).
// In place is y == z, so neither pointer is __restrict__: a thread reads its 16 bytes before it writes them, and no other thread
// touches them.
static __global__ __launch_bounds__(256) void bn_apply_kernel(const float* z, int64_t ldz, int64_t rows, int C,
                                                       const float* __restrict__ affine, int relu, float* y, int64_t ldy) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int c4 = C / 4;
  if (i >= rows * c4) return;
  const int64_t r = i / c4;
  const int c = (int)(i - r * c4) * 4;
  f32x4 v = *reinterpret_cast<const f32x4*>(z + r * ldz + c);
  const f32x4 a = *reinterpret_cast<const f32x4*>(affine + c), b = *reinterpret_cast<const f32x4*>(affine + C + c);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
#pragma clang fp contract(off)
    const float t = v[k] * a[k] + b[k];
    v[k] = relu ? fmaxf(t, 0.f) : t;
  }
  *reinterpret_cast<f32x4*>(y + r * ldy + c) = v;
}

// row chunks (blocks of bn_partial_kernel) for `rows` rows: one per 64 rows, at most BN_MAX_BLOCKS
inline int bn_row_chunks(int64_t rows) { return (int)std::min<int64_t>(BN_MAX_BLOCKS, std::max<int64_t>(1, rows / 64)); }

// What the kernels here and in lt_bnbwd.h are written for: channels in quads that the statistics scratch holds, and rows [*][C] that
// a thread moves 16 bytes at a time (bn_partial_kernel takes its stride as an int).  Every caller refuses the rest before it launches.
inline bool bn_channels_ok(int C) { return C >= 4 && C <= BN_MAX_CHANNELS && C % 4 == 0; }
inline bool bn_rows_ok(const void* base, int64_t ld, int C) { return ld >= C && ld % 4 == 0 && ld <= INT32_MAX && (uintptr_t)base % 16 == 0; }

// The BatchNorm forward on rows > 0 rows that passed the two predicates: statistics (train mode), coefficients, transform.
// partial [bn_row_chunks(rows)][2 C] and affine [2 C] are scratch; running, batch and save as in bn_finalize_kernel; y may be z.
// h (may be null) only names the profile scopes.
inline int bn_forward_launch(hipStream_t st, LinetrHandle* h, double* partial, float* affine, const float* z, int64_t ldz, int64_t rows,
                             int C, const float* gamma, const float* beta, float eps, float momentum, float* running, bool eval,
                             float* batch, double* save, bool relu, float* y, int64_t ldy) {
  const int nb = bn_row_chunks(rows);
  if (!eval) {
    ProfScope ps(h, st, "bn_fwd_partial", 0, 4.0 * rows * C);
    hipLaunchKernelGGL(bn_partial_kernel, dim3(nb), dim3(256), 0, st, z, rows, C, (int)ldz, partial);
    LT_LAUNCH_CHECK();
  }
  {
    ProfScope ps(h, st, "bn_fwd_finalize", 0, 16.0 * nb * C);
    hipLaunchKernelGGL(bn_finalize_kernel, dim3((C + 255) / 256), dim3(256), 0, st, (const double*)partial, nb, C, rows, gamma, beta, eps,
                       momentum, running, (int)eval, batch, affine, save);
    LT_LAUNCH_CHECK();
  }
  {
    ProfScope ps(h, st, "bn_fwd_apply", 0, 8.0 * rows * C);
    hipLaunchKernelGGL(bn_apply_kernel, dim3((unsigned)((rows * (C / 4) + 255) / 256)), dim3(256), 0, st, z, ldz, rows, C,
                       (const float*)affine, (int)relu, y, ldy);
    LT_LAUNCH_CHECK();
  }
  return LINETR_OK;
}

// BatchNorm(train) + ReLU in place on z [rows][C]; `off` = float offset of the layer inside the packed statistics
// `nb_used` (may be null) receives the number of row chunks (linetr_debug_bn_train)
inline int bn_train_layer(hipStream_t st, const BnTrain& bt, float* z, int64_t rows, int C, int ld, const float* gamma,
                          const float* beta, int64_t off, int* nb_used = nullptr) {
  if (nb_used) *nb_used = 0;
  if (rows <= 0) return 0;
  if (!bn_channels_ok(C))
    return fail(LINETR_E_ARG, "BatchNorm(train): %d channels (the statistics scratch holds 4 .. %d, multiples of 4)", C, BN_MAX_CHANNELS);
  if (!bn_rows_ok(z, ld, C))
    return fail(LINETR_E_ARG, "BatchNorm(train): rows of %d channels need a row stride >= %d that is a multiple of 4 (got %d) and a 16-byte aligned base", C, C, ld);
  if (nb_used) *nb_used = bn_row_chunks(rows);
  return bn_forward_launch(st, nullptr, bt.partial, bt.affine, z, ld, rows, C, gamma, beta, 1e-5f, bt.momentum, bt.running + off, false,
                           bt.batch ? bt.batch + off : nullptr, nullptr, true, z, ld);
}

}  // namespace lt
