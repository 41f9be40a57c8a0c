// Device pieces that kernels of more than one translation unit use (a kernel header belongs to ONE unit: its kernels are not inline):
// the exact-fp32 64 x 64 dot tile (the matcher, lt_match.h, and the criterion, lt_valstep.h / lt_lossgrad.h) and the block-wide
// exclusive scan (the key-point branch, lt_keypoints.h, and the ground-truth match list, lt_gtassign.h).
#pragma once
#include "lt_common.h"

namespace lt {

// One 64 x 64 tile of dot products <A[a0 + .], B[b0 + .]> over K = 256 by exact-fp32 MFMA (v_mfma_f32_32x32x2_f32: a k-ordered fmaf
// chain, no split) for a block of 4 waves: wave (wa, wb) owns the 32 x 32 quarter at (32 wa, 32 wb).  As / Bs: [64 * DOT_LS] floats of
// LDS each.  Rows beyond n0 / n1 are read as the last row (their results are the caller's to drop).  Element r of the result is
// row dot_tile_row(r, lane), column lane & 31 of the quarter.
constexpr int DOT_LS = 36;
__device__ __forceinline__ int dot_tile_row(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }
__device__ __forceinline__ f32x16 dot_tile_64x64(const float* __restrict__ A, int n0, int a0, const float* __restrict__ B, int n1, int b0,
                                                 float* As, float* Bs) {
  constexpr int LS = DOT_LS;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wa = wave >> 1, wb = wave & 1;
  const int lrow = tid >> 3, lc4 = (tid & 7) * 4;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  // rows of this thread's staging pieces; the NEXT K tile travels in registers while the current one is multiplied
  int ra[2], rb[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    ra[i] = a0 + lrow + i * 32; ra[i] = ra[i] < n0 ? ra[i] : n0 - 1;
    rb[i] = b0 + lrow + i * 32; rb[i] = rb[i] < n1 ? rb[i] : n1 - 1;
  }
  f32x4 va[2], vb[2];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      va[i] = *reinterpret_cast<const f32x4*>(A + (int64_t)ra[i] * D + k0 + lc4);
      vb[i] = *reinterpret_cast<const f32x4*>(B + (int64_t)rb[i] * D + k0 + lc4);
    }
  };
  fetch(0);
  for (int k0 = 0; k0 < D; k0 += 32) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      *reinterpret_cast<f32x4*>(&As[(lrow + i * 32) * LS + lc4]) = va[i];
      *reinterpret_cast<f32x4*>(&Bs[(lrow + i * 32) * LS + lc4]) = vb[i];
    }
    if (k0 + 32 < D) fetch(k0 + 32);
    __syncthreads();
    const float* ap = &As[(wa * 32 + (lane & 31)) * LS + (lane >> 5) * 4];
    const float* bp = &Bs[(wb * 32 + (lane & 31)) * LS + (lane >> 5) * 4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(ap + kk * 8);
      const f32x4 b = *reinterpret_cast<const f32x4*>(bp + kk * 8);
#pragma unroll
      for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], b[s], acc, 0, 0, 0);
    }
  }
  return acc;
}

// exclusive scan over up to 256 values per pass, one per thread; returns the thread's exclusive prefix and the total in `sum`
__device__ __forceinline__ int kp_block_scan(int c, int* part, int& sum) {
  const int t = threadIdx.x;
  part[t] = c;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {
    const int v = t >= off ? part[t - off] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  const int inc = part[t];
  sum = part[255];
  __syncthreads();
  return inc - c;
}

}  // namespace lt
