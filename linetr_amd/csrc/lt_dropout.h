// Training-time dropout of the line descriptive layer (the reference's three nn.Dropout(0.1), models/line_attention.py:18, :70, :90), in
// the folded form of lt_descbwd.h: siblings of cp_fwd_kernel / cp_bwd_kernel / ln_fwd_kernel / ln_bwd_kernel that generate their masks
// themselves.  A mask is a pure function of (seed, call, site, row, element): Philox4x32-10, key = (seed lo, seed hi), counter =
// (inner, row, call, site); a word w keeps its element iff w >= threshold = floor(p 2^32), and the factor r is scale = 1 / (1 - p) or 0.
// The backward kernels generate the same words again: no mask is stored, and the bits do not depend on the launch geometry.
//
//   site 0, the attention weights of the CLS query row: inner = token t, word h belongs to head h -- one Philox call per token, on
//     wave-uniform inputs (the segment is one wave's, read through readfirstlane), so it runs on the scalar unit, not 64 times per wave.
//     a_t = p_t r_t    pooled_h = sum_t a_t x_t    kept_h = sum_t a_t  (the value bias then enters as kept_h bv_h; no dropout: kept = 1)
//     da_t = dpooled_h . x_t + dkept_h    delta_h = dpooled_h . pooled_h + dkept_h kept_h    ds_t = p_t (r_t da_t - delta_h)
//     dx_t = sum_h (a_t dpooled_h + ds_t u_h)    du_h = sum_t ds_t x_t
//     (r_t da_t is formed as dpooled_h . fl(scale x_t) + scale dkept_h for a kept token and 0 for a dropped one: the roundings of delta_h,
//     so that at S = 1, where ds = 0 in exact arithmetic, the two are the same number and du is exactly 0, as in cp_bwd_kernel)
//     A (segment, head) whose tokens are all dropped: pooled = 0 and kept = 0 exactly, ds = 0, no NaN (lse is that of the full softmax).
//   sites 1, 2, in front of the two residual LayerNorms: inner = column / 4, word k belongs to column 4 inner + k -- one call per lane.
//     v = fl(r a) + residual (two roundings: the bits of the plain kernels on a pre-masked a)    y = LN(v)
//     backward: dv as ln_bwd_kernel's dx;  dresidual = dv,  da = r dv
// threshold 0 (p = 0) keeps every element with the factor `scale`; with scale = 1 every output has the bits of the plain kernels.
// Deterministic as lt_descbwd.h: no atomics, every sum in a fixed order, nothing at or beyond the last row is loaded or stored.
#pragma once
#include "lt_descbwd.h"

namespace lt {

struct DropArgs {          // LinetrDropout as the kernels take it
  uint32_t key0, key1, call, threshold;
  float scale;
};

// Philox4x32-10 (Salmon et al., SC'11), the standard multipliers and key increments
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t (&w)[4]) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}

// the four factors of (inner, row) at `site`
__device__ __forceinline__ void drop_factors(const DropArgs& dr, uint32_t site, uint32_t row, uint32_t inner, float (&f)[4]) {
  uint32_t w[4];
  philox4x32_10(inner, row, dr.call, site, dr.key0, dr.key1, w);
#pragma unroll
  for (int k = 0; k < 4; ++k) f[k] = w[k] >= dr.threshold ? dr.scale : 0.f;
}

// fl(a f): its own rounding, never fused into the residual add behind it
__device__ __forceinline__ f32x4 drop_apply(const f32x4 a, const float (&f)[4]) {
#pragma clang fp contract(off)
  return f32x4{a[0] * f[0], a[1] * f[1], a[2] * f[2], a[3] * f[3]};
}
// fl(a b) likewise
__device__ __forceinline__ f32x4 mul_rounded(const f32x4 a, const f32x4 b) {
#pragma clang fp contract(off)
  return a * b;
}

// grid ceil(n / 256), 256 threads; out [rows][inner][4]: the factors themselves (tests, debugging)
__global__ __launch_bounds__(256) void drop_factors_kernel(DropArgs dr, uint32_t site, int64_t rows, int64_t inner, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * inner) return;
  const int64_t row = i / inner;
  float f[4];
  drop_factors(dr, site, (uint32_t)row, (uint32_t)(i - row * inner), f);
  *reinterpret_cast<f32x4*>(out + i * 4) = f32x4{f[0], f[1], f[2], f[3]};
}

// cp_fwd_kernel with site 0's factors on the softmax weights; kept [L][4]
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

// cp_bwd_kernel with site 0's factors generated again; dkept [L][4] may be null (no gradient arrives at kept)
__global__ __launch_bounds__(256) void cp_drop_bwd_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ u, int64_t ldu,
                                                          const float* __restrict__ pooled, const float* __restrict__ lse,
                                                          const float* __restrict__ kept, const float* __restrict__ dpooled,
                                                          const float* __restrict__ dkept, int64_t L, int S, DropArgs dr,
                                                          float* __restrict__ dx, int64_t lddx, float* __restrict__ du, int64_t lddu) {
  const int lane = threadIdx.x & 63;
  const int64_t l = (int64_t)blockIdx.x * CP_SEGS + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (l >= L) return;
  const int c = lane * 4;
  f32x4 uh[HEADS], dph[HEADS], duh[HEADS];
  float delta[HEADS], ls[HEADS], dk[HEADS];
#pragma unroll
  for (int h = 0; h < HEADS; ++h) {
    uh[h] = *reinterpret_cast<const f32x4*>(u + l * ldu + h * D + c);
    dph[h] = *reinterpret_cast<const f32x4*>(dpooled + l * (HEADS * D) + h * D + c);
    const f32x4 ph = *reinterpret_cast<const f32x4*>(pooled + l * (HEADS * D) + h * D + c);
    duh[h] = f32x4{0.f, 0.f, 0.f, 0.f};
    delta[h] = dot4(dph[h], ph);
    ls[h] = lse[l * HEADS + h];
    dk[h] = dkept ? dkept[l * HEADS + h] : 0.f;
  }
  wave_sum_n(delta);
  if (dkept) {
#pragma unroll
    for (int h = 0; h < HEADS; ++h) delta[h] = fmaf(dk[h], kept[l * HEADS + h], delta[h]);
  }
  const float* xs = x + l * S * ldx + c;
  float* dxs = dx ? dx + l * S * lddx + c : nullptr;
  for (int t0 = 0; t0 < S; t0 += CP_TOK_B) {
    f32x4 xv[CP_TOK_B];
    float s[CP_TOK_B * 2 * HEADS], r[CP_TOK_B][HEADS];
#pragma unroll
    for (int j = 0; j < CP_TOK_B; ++j)
      xv[j] = t0 + j < S ? *reinterpret_cast<const f32x4*>(xs + (int64_t)(t0 + j) * ldx) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < CP_TOK_B; ++j) drop_factors(dr, 0u, (uint32_t)l, (uint32_t)(t0 + j), r[j]);
#pragma unroll
    for (int j = 0; j < CP_TOK_B; ++j) {
      const f32x4 xs = xv[j] * dr.scale;                    // a kept token as the forward pooled it: at S = 1 it IS pooled, bit for bit
#pragma unroll
      for (int h = 0; h < HEADS; ++h) {
        s[(j * 2) * HEADS + h] = dot4(uh[h], xv[j]);
        s[(j * 2 + 1) * HEADS + h] = dot4(dph[h], xs);
      }
    }
    wave_sum_n(s);
#pragma unroll
    for (int j = 0; j < CP_TOK_B; ++j) {
      if (t0 + j >= S) break;
      f32x4 out = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int h = 0; h < HEADS; ++h) {
        const float p = expf(s[(j * 2) * HEADS + h] - ls[h]);
        const float a = p * r[j][h];
        // r da = scale (dpooled . x + dkept) for a kept token, rounded as delta is: at S = 1 both are the same number and ds = 0
        const float sda = dkept ? fmaf(dk[h], dr.scale, s[(j * 2 + 1) * HEADS + h]) : s[(j * 2 + 1) * HEADS + h];
        const float ds = p * ((r[j][h] != 0.f ? sda : 0.f) - delta[h]);
        out += dph[h] * a + uh[h] * ds;
        duh[h] += xv[j] * ds;
      }
      if (dxs) *reinterpret_cast<f32x4*>(dxs + (int64_t)(t0 + j) * lddx) = out;
    }
  }
  if (du) {
#pragma unroll
    for (int h = 0; h < HEADS; ++h) *reinterpret_cast<f32x4*>(du + l * lddu + h * D + c) = duh[h];
  }
}

// ln_fwd_kernel on v = fl(r a) + residual, r the factors of `site` (1 or 2)
__global__ __launch_bounds__(256) void ln_drop_fwd_kernel(const float* __restrict__ a, int64_t lda, const float* __restrict__ r, int64_t ldr,
                                                          const float* __restrict__ gamma, const float* __restrict__ beta, float eps, int64_t rows,
                                                          DropArgs dr, uint32_t site, float* __restrict__ y, int64_t ldy, float* __restrict__ stats) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * LN_ROWS + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int c = lane * 4;
  float f[4];
  drop_factors(dr, site, (uint32_t)row, (uint32_t)lane, f);
  f32x4 v = drop_apply(*reinterpret_cast<const f32x4*>(a + row * lda + c), f);
  if (r) v += *reinterpret_cast<const f32x4*>(r + row * ldr + c);
  f32x4 d;
  float mean, rstd;
  ln_row_stats(v, eps, d, mean, rstd);
  const f32x4 gm = *reinterpret_cast<const f32x4*>(gamma + c), bt = *reinterpret_cast<const f32x4*>(beta + c);
  *reinterpret_cast<f32x4*>(y + row * ldy + c) = (d * rstd) * gm + bt;
  if (lane == 0) { stats[row * 2] = mean; stats[row * 2 + 1] = rstd; }
}

// ln_bwd_kernel on the same v: dres <- dv, da <- r dv (each may be null); partial as ln_bwd_kernel's
__global__ __launch_bounds__(256) void ln_drop_bwd_kernel(const float* __restrict__ a, int64_t lda, const float* __restrict__ r, int64_t ldr,
                                                          const float* __restrict__ stats, const float* __restrict__ gamma,
                                                          const float* __restrict__ g, int64_t ldg, int64_t rows, DropArgs dr, uint32_t site,
                                                          float* __restrict__ da, int64_t ldda, float* __restrict__ dres, int64_t lddr,
                                                          float* __restrict__ partial) {
  __shared__ f32x4 red[3][2][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = lane * 4;
  const int64_t r0 = (int64_t)blockIdx.x * LN_CHUNK;
  const int64_t r1 = r0 + LN_CHUNK < rows ? r0 + LN_CHUNK : rows;
  const f32x4 gm = *reinterpret_cast<const f32x4*>(gamma + c);
  f32x4 dg = f32x4{0.f, 0.f, 0.f, 0.f}, db = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int64_t row = r0 + wave; row < r1; row += 4) {
    float f[4];
    drop_factors(dr, site, (uint32_t)row, (uint32_t)lane, f);
    f32x4 v = drop_apply(*reinterpret_cast<const f32x4*>(a + row * lda + c), f);
    if (r) v += *reinterpret_cast<const f32x4*>(r + row * ldr + c);
    const f32x4 gv = *reinterpret_cast<const f32x4*>(g + row * ldg + c);
    const float mean = stats[row * 2], rstd = stats[row * 2 + 1];
    const f32x4 xh = (v - mean) * rstd;
    const f32x4 gg = mul_rounded(gv, gm);                  // (ln_bwd_kernel rounds g gamma before it subtracts the mean)
    // (the fmas of ln_bwd_kernel's compiled text, written out: dv must have its bits)
    float s[2] = {(gg[0] + gg[1]) + (gg[2] + gg[3]), fmaf(gg[0], xh[0], gg[1] * xh[1]) + fmaf(gg[2], xh[2], gg[3] * xh[3])};
    wave_sum_n(s);
    const float c1 = s[0] * (1.f / D), c2 = s[1] * (1.f / D);
    const f32x4 t = gg - c1;
    const f32x4 dv = f32x4{fmaf(-xh[0], c2, t[0]), fmaf(-xh[1], c2, t[1]), fmaf(-xh[2], c2, t[2]), fmaf(-xh[3], c2, t[3])} * rstd;
    if (dres) *reinterpret_cast<f32x4*>(dres + row * lddr + c) = dv;
    if (da) *reinterpret_cast<f32x4*>(da + row * ldda + c) = drop_apply(dv, f);
    dg = f32x4{fmaf(gv[0], xh[0], dg[0]), fmaf(gv[1], xh[1], dg[1]), fmaf(gv[2], xh[2], dg[2]), fmaf(gv[3], xh[3], dg[3])};
    db += gv;
  }
  if (!partial) return;
  if (wave > 0) { red[wave - 1][0][lane] = dg; red[wave - 1][1][lane] = db; }
  __syncthreads();
  if (wave == 0) {
#pragma unroll
    for (int w = 0; w < 3; ++w) { dg += red[w][0][lane]; db += red[w][1][lane]; }     // wave order
    float* out = partial + (int64_t)blockIdx.x * (2 * D);
    *reinterpret_cast<f32x4*>(out + c) = dg;
    *reinterpret_cast<f32x4*>(out + D + c) = db;
  }
}

}  // namespace lt
