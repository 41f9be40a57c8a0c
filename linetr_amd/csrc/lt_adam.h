// The optimizer step of the reference's training iteration (train.py:82, :195: torch.optim.Adam) and the gradient norm that can feed it,
// over a TABLE of tensors in one launch.  The table (LinetrAdamTensor, include/linetr_hip.h) lives in device memory behind a prefix of
// chunk counts: tensor t owns the blocks prefix[t] .. prefix[t + 1] - 1, each block one chunk of AD_CHUNK elements of it.  A block finds
// its tensor by a binary search of the prefix on block-uniform values (scalar loads, scalar registers); a tensor of no elements owns no
// block and is never found.  The table reaches the device through the kernel arguments of ad_table_kernel, AD_PIECE entries a launch:
// the runtime copies kernel arguments when the launch is queued, so the host table may change or vanish as soon as the call returns,
// nothing on the host is kept and nothing waits, whatever the runtime does with copies out of pageable memory.
//
// The update, per element, float32, one rounding per written operation, in the order of torch's _single_tensor_adam (torch 2.10,
// non-capturable):
//   g  <- fl(scale g)                          only with a scale pointer (one float32 read on the device); rounded on its own
//   mode 1 (coupled weight decay)    g <- fmaf(wd, p, g)
//   mode 2 (decoupled weight decay)  p <- fl(p decay)            decay = float(1 - lr wd)
//   m' = fmaf(b1c, g - m, m)                   b1c = float(1 - beta1)
//   v' = fmaf(fl(b2c g), g, fl(b2 v))          b2c = float(1 - beta2), b2 = float(beta2)
//   d  = sqrtf(v') / bc2_sqrt + eps            IEEE square root and division
//   p' = fmaf(-step_size, m' / d, p)
// Contraction is off in ad_update: the compiler fuses nothing that is not written as an fmaf.
// Memory: 16 bytes a lane where p, g, m and v of the tensor are all 16-byte aligned (a chunk starts at a multiple of 4 elements, so the
// tensor's alignment is the chunk's), with a scalar tail; 4 bytes a lane otherwise.  No LDS, no atomics, no block talks to another;
// nothing outside [0, n) of a tensor is loaded or stored.
//
// The norm: gn_partial_kernel sums the squares of one chunk of g in float64 (a float32 square is exact there) -- lane t adds elements
// t, t + 256, ... in ascending order, the lanes of a wave are added by a fixed shuffle tree, the four waves in ascending order -- and
// gn_final_kernel, one block, adds the chunks' sums: 256 contiguous runs, each in ascending order, then the runs in ascending order.
// The order depends on nothing but the table's sizes: not on alignment, not on timing.
#pragma once
#include "lt_common.h"

namespace lt {

constexpr int AD_CHUNK = 4096;     // elements a block updates
constexpr int AD_THREADS = 256;
constexpr int AD_PIECE = 64;       // table entries one ad_table_kernel launch carries in its arguments (64 * 48 + 65 * 4 bytes < 4 KB)

struct AdamK {                     // LinetrAdamHyper as the kernel takes it
  float b1c, b2c, b2, eps, wd, decay;
  int mode;                        // 0: no weight decay, 1: coupled, 2: decoupled
};

struct AdamTablePiece {
  LinetrAdamTensor entry[AD_PIECE];
  int32_t prefix[AD_PIECE + 1];    // prefix[count]: written by the last piece alone (it is the next piece's prefix[0] otherwise)
};

// grid 1, 64 threads: table[first + i] and prefix[first + i] for i < count, and the closing prefix[first + count] where `last`
__global__ __launch_bounds__(AD_PIECE) void ad_table_kernel(const AdamTablePiece piece, int first, int count, int last,
                                                            LinetrAdamTensor* __restrict__ table, int32_t* __restrict__ prefix) {
  const int i = threadIdx.x;
  if (i < count) {
    table[first + i] = piece.entry[i];
    prefix[first + i] = piece.prefix[i];
  }
  if (i == 0 && last) prefix[first + count] = piece.prefix[count];
}

// the tensor that owns block b: the t with prefix[t] <= b < prefix[t + 1] (prefix[0] = 0 <= b < prefix[n_tensors] for every block launched)
__device__ __forceinline__ int ad_find_tensor(const int32_t* __restrict__ prefix, int n_tensors, int b) {
  int lo = 0, hi = n_tensors;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (prefix[mid] <= b) lo = mid; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ void ad_update(float& p, float g, float& m, float& v, const AdamK& k, float step_size, float bc2_sqrt,
                                          bool scaled, float scale) {
#pragma clang fp contract(off)
  if (scaled) g = scale * g;
  if (k.mode == 1) g = fmaf(k.wd, p, g);
  if (k.mode == 2) p = p * k.decay;
  m = fmaf(k.b1c, g - m, m);
  const float a = k.b2c * g, c = k.b2 * v;
  v = fmaf(a, g, c);
  const float d = sqrtf(v) / bc2_sqrt + k.eps;
  p = fmaf(-step_size, m / d, p);
}

// grid prefix[n_tensors] (one block a chunk), 256 threads
__global__ __launch_bounds__(AD_THREADS) void ad_step_kernel(const LinetrAdamTensor* __restrict__ table, const int32_t* __restrict__ prefix,
                                                             int n_tensors, const AdamK k, const float* __restrict__ d_scale) {
  const int b = blockIdx.x;
  const int t = ad_find_tensor(prefix, n_tensors, b);
  const LinetrAdamTensor e = table[t];
  const int64_t base = (int64_t)(b - prefix[t]) * AD_CHUNK;
  const int len = (int)(e.n - base < AD_CHUNK ? e.n - base : AD_CHUNK);
  float* __restrict__ p = e.p + base;
  const float* __restrict__ g = e.g + base;
  float* __restrict__ m = e.m + base;
  float* __restrict__ v = e.v + base;
  const bool scaled = d_scale != nullptr;
  const float scale = scaled ? *d_scale : 1.f;
  const int tid = threadIdx.x;
  if ((((uintptr_t)e.p | (uintptr_t)e.g | (uintptr_t)e.m | (uintptr_t)e.v) & 15) == 0) {
    const int quads = len >> 2;
    for (int q = tid; q < quads; q += AD_THREADS) {
      f32x4 pv = reinterpret_cast<const f32x4*>(p)[q];
      const f32x4 gv = reinterpret_cast<const f32x4*>(g)[q];
      f32x4 mv = reinterpret_cast<const f32x4*>(m)[q];
      f32x4 vv = reinterpret_cast<const f32x4*>(v)[q];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float pj = pv[j], mj = mv[j], vj = vv[j];
        ad_update(pj, gv[j], mj, vj, k, e.step_size, e.bc2_sqrt, scaled, scale);
        pv[j] = pj; mv[j] = mj; vv[j] = vj;
      }
      reinterpret_cast<f32x4*>(p)[q] = pv;
      reinterpret_cast<f32x4*>(m)[q] = mv;
      reinterpret_cast<f32x4*>(v)[q] = vv;
    }
    const int i = (quads << 2) + tid;        // the scalar tail: at most 3 elements
    if (i < len) {
      float pj = p[i], mj = m[i], vj = v[i];
      ad_update(pj, g[i], mj, vj, k, e.step_size, e.bc2_sqrt, scaled, scale);
      p[i] = pj; m[i] = mj; v[i] = vj;
    }
  } else {
    for (int i = tid; i < len; i += AD_THREADS) {
      float pj = p[i], mj = m[i], vj = v[i];
      ad_update(pj, g[i], mj, vj, k, e.step_size, e.bc2_sqrt, scaled, scale);
      p[i] = pj; m[i] = mj; v[i] = vj;
    }
  }
}

// grid prefix[n_tensors], 256 threads: partial[b] = the sum of squares of block b's chunk of g, float64
__global__ __launch_bounds__(AD_THREADS) void gn_partial_kernel(const LinetrAdamTensor* __restrict__ table, const int32_t* __restrict__ prefix,
                                                                int n_tensors, double* __restrict__ partial) {
  __shared__ double s_wave[AD_THREADS / 64];
  const int b = blockIdx.x;
  const int t = ad_find_tensor(prefix, n_tensors, b);
  const LinetrAdamTensor e = table[t];
  const int64_t base = (int64_t)(b - prefix[t]) * AD_CHUNK;
  const int len = (int)(e.n - base < AD_CHUNK ? e.n - base : AD_CHUNK);
  const float* __restrict__ g = e.g + base;
  double acc = 0.0;
  for (int i = threadIdx.x; i < len; i += AD_THREADS) {
    const double x = (double)g[i];
    acc = fma(x, x, acc);
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) acc += __shfl_down(acc, off, 64);
  if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partial[b] = ((s_wave[0] + s_wave[1]) + s_wave[2]) + s_wave[3];
}

// grid 1, 256 threads: norm = sqrt(sum of the partials), scale = float(min(1, max_norm / (norm + 1e-6))) -- clip_grad_norm_'s coefficient;
// a NaN norm gives a NaN scale, as torch's clamp does
__global__ __launch_bounds__(AD_THREADS) void gn_final_kernel(const double* __restrict__ partial, int chunks, double max_norm,
                                                              double* __restrict__ d_norm, float* __restrict__ d_scale) {
  __shared__ double s_run[AD_THREADS];
  const int per = (chunks + AD_THREADS - 1) / AD_THREADS;
  const int lo = threadIdx.x * per;
  const int hi = lo + per < chunks ? lo + per : chunks;
  double acc = 0.0;
  for (int i = lo; i < hi; ++i) acc += partial[i];
  s_run[threadIdx.x] = acc;
  __syncthreads();
  if (threadIdx.x != 0) return;
  double total = 0.0;
  for (int i = 0; i < AD_THREADS; ++i) total += s_run[i];
  const double norm = sqrt(total);
  const double coef = max_norm / (norm + 1e-6);
  d_norm[0] = norm;
  d_scale[0] = (float)(coef < 1.0 ? coef : (coef != coef ? coef : 1.0));
}

}  // namespace lt
