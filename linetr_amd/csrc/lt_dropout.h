// Training-time dropout of the line descriptive layer (the reference's three nn.Dropout(0.1), models/line_attention.py:18, :70, :90), in
// the folded form of lt_descbwd.h: the DROP instances of its three bodies (cp_bwd_body / ln_fwd_body / ln_bwd_body) and a copy of its
// pooling forward, which generate their masks themselves.  A mask is a pure function of (seed, call, site, row, element):
// Philox4x32-10, key = (seed lo, seed hi), counter = (inner, row, call, site); a word w keeps its element iff w >= threshold =
// floor(p 2^32), and the factor r is scale = 1 / (1 - p) or 0.  The backward kernels generate the same words again: no mask is stored,
// and the bits do not depend on the launch geometry.
//
//   site 0, the attention weights of the CLS query row: inner = token t, word h belongs to head h -- one Philox call per token, on
//     wave-uniform inputs (the segment is one wave's, read through readfirstlane), so it runs on the scalar unit, not 64 times per wave.
//     a_t = p_t r_t    pooled_h = sum_t a_t x_t    kept_h = sum_t a_t  (the value bias then enters as kept_h bv_h; no dropout: kept = 1)
//     da_t = dpooled_h . x_t + dkept_h    delta_h = dpooled_h . pooled_h + dkept_h kept_h    ds_t = p_t (r_t da_t - delta_h)
//     dx_t = sum_h (a_t dpooled_h + ds_t u_h)    du_h = sum_t ds_t x_t
//     (r_t da_t is formed as dpooled_h . fl(scale x_t) + scale dkept_h for a kept token and 0 for a dropped one: the roundings of delta_h,
//     so that at S = 1, where ds = 0 in exact arithmetic, the two are the same number and du is exactly 0, as without dropout)
//     A (segment, head) whose tokens are all dropped: pooled = 0 and kept = 0 exactly, ds = 0, no NaN (lse is that of the full softmax).
//   sites 1, 2, in front of the two residual LayerNorms: inner = column / 4, word k belongs to column 4 inner + k -- one call per lane.
//     v = fl(r a) + residual (two roundings: the bits of the plain instance on a pre-masked a)    y = LN(v)
//     backward: dv as without dropout;  dresidual = dv,  da = r dv
// threshold 0 (p = 0) keeps every element with the factor `scale`; with scale = 1 every output has the bits of the plain instance: the
// statements a body has under DROP then multiply by 1, add 0 or select what the plain text takes.
// Deterministic as lt_descbwd.h: no atomics, every sum in a fixed order, nothing at or beyond the last row is loaded or stored.
#pragma once
#include "lt_descbwd.h"

namespace lt {

// grid ceil(n / 256), 256 threads; out [rows][inner][4]: the factors themselves (tests, debugging)
__global__ __launch_bounds__(256) void drop_factors_kernel(DropArgs dr, uint32_t site, int64_t rows, int64_t inner, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * inner) return;
  const int64_t row = i / inner;
  float f[4];
  drop_factors(dr, site, (uint32_t)row, (uint32_t)(i - row * inner), f);
  *reinterpret_cast<f32x4*>(out + i * 4) = f32x4{f[0], f[1], f[2], f[3]};
}

// cp_fwd_kernel with site 0's factors on the softmax weights; kept [L][4].  A copy of cp_fwd_kernel's text with r, pr and kept added,
// not an instance of one body: called through an inlined body, this kernel took 1.04 of its time on the MI355X, in every repetition
// (profiles/desc_drop_once_bench.txt).  A change to the online softmax is made in both.
__global__ __launch_bounds__(256) void cp_drop_fwd_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ u, int64_t ldu,
                                                          int64_t L, int S, DropArgs dr, float* __restrict__ pooled, float* __restrict__ kept,
                                                          float* __restrict__ lse) {
  const int lane = threadIdx.x & 63;
  const int64_t l = (int64_t)blockIdx.x * CP_SEGS + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);       // (wave-uniform, provably)
  if (l >= L) return;
  const int c = lane * 4;
  f32x4 uh[HEADS], acc[HEADS];
  float m[HEADS], den[HEADS], kd[HEADS];
#pragma unroll
  for (int h = 0; h < HEADS; ++h) {
    uh[h] = *reinterpret_cast<const f32x4*>(u + l * ldu + h * D + c);
    acc[h] = f32x4{0.f, 0.f, 0.f, 0.f};
    m[h] = -INFINITY;
    den[h] = 0.f;
    kd[h] = 0.f;
  }
  const float* xs = x + l * S * ldx + c;
  for (int t0 = 0; t0 < S; t0 += CP_TOK) {
    f32x4 xv[CP_TOK];
    float s[CP_TOK * HEADS], r[CP_TOK][HEADS];
#pragma unroll
    for (int j = 0; j < CP_TOK; ++j)
      xv[j] = t0 + j < S ? *reinterpret_cast<const f32x4*>(xs + (int64_t)(t0 + j) * ldx) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < CP_TOK; ++j) drop_factors(dr, 0u, (uint32_t)l, (uint32_t)(t0 + j), r[j]);
#pragma unroll
    for (int j = 0; j < CP_TOK; ++j)
#pragma unroll
      for (int h = 0; h < HEADS; ++h) s[j * HEADS + h] = dot4(uh[h], xv[j]);
    wave_sum_n(s);
#pragma unroll
    for (int h = 0; h < HEADS; ++h) {
      float mx = m[h];
#pragma unroll
      for (int j = 0; j < CP_TOK; ++j) {
        if (t0 + j >= S) s[j * HEADS + h] = -INFINITY;       // (token 0 of a chunk exists: mx is finite below)
        mx = fmaxf(mx, s[j * HEADS + h]);
      }
      const float scale = expf(m[h] - mx);                  // exp(-inf) = 0 at the first chunk
      float d = den[h] * scale, k = kd[h] * scale;
      f32x4 a = acc[h] * scale;
#pragma unroll
      for (int j = 0; j < CP_TOK; ++j) {
        const float p = expf(s[j * HEADS + h] - mx);
        const float pr = p * r[j][h];
        d += p;
        k += pr;
        a += xv[j] * pr;
      }
      m[h] = mx;
      den[h] = d;
      kd[h] = k;
      acc[h] = a;
    }
  }
#pragma unroll
  for (int h = 0; h < HEADS; ++h) {
    const float inv = 1.f / den[h];
    *reinterpret_cast<f32x4*>(pooled + l * (HEADS * D) + h * D + c) = acc[h] * inv;
    kd[h] *= inv;
  }
  if (lane < HEADS) {
    float v = 0.f, k = 0.f;
#pragma unroll
    for (int h = 0; h < HEADS; ++h) {
      v = lane == h ? m[h] + logf(den[h]) : v;
      k = lane == h ? kd[h] : k;
    }
    lse[l * HEADS + lane] = v;
    kept[l * HEADS + lane] = k;
  }
}

// The DROP instances of the bodies of lt_descbwd.h; grids and arguments as its plain kernels; kept, dkept [L][4]; site 1 or 2
__global__ __launch_bounds__(256) void cp_drop_bwd_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ u, int64_t ldu,
                                                          const float* __restrict__ pooled, const float* __restrict__ lse,
                                                          const float* __restrict__ kept, const float* __restrict__ dpooled,
                                                          const float* __restrict__ dkept, int64_t L, int S, DropArgs dr,
                                                          float* __restrict__ dx, int64_t lddx, float* __restrict__ du, int64_t lddu) {
  cp_bwd_body<true>(x, ldx, u, ldu, pooled, lse, kept, dpooled, dkept, L, S, dr, dx, lddx, du, lddu);
}

__global__ __launch_bounds__(256) void ln_drop_fwd_kernel(const float* __restrict__ a, int64_t lda, const float* __restrict__ r, int64_t ldr,
                                                          const float* __restrict__ gamma, const float* __restrict__ beta, float eps, int64_t rows,
                                                          DropArgs dr, uint32_t site, float* __restrict__ y, int64_t ldy, float* __restrict__ stats) {
  ln_fwd_body<true>(a, lda, r, ldr, gamma, beta, eps, rows, dr, site, y, ldy, stats);
}

__global__ __launch_bounds__(256) void ln_drop_bwd_kernel(const float* __restrict__ a, int64_t lda, const float* __restrict__ r, int64_t ldr,
                                                          const float* __restrict__ stats, const float* __restrict__ gamma,
                                                          const float* __restrict__ g, int64_t ldg, int64_t rows, DropArgs dr, uint32_t site,
                                                          float* __restrict__ da, int64_t ldda, float* __restrict__ dres, int64_t lddr,
                                                          float* __restrict__ partial) {
  ln_bwd_body<true>(a, lda, r, ldr, stats, gamma, g, ldg, rows, dr, site, da, ldda, dres, lddr, partial);
}

}  // namespace lt
