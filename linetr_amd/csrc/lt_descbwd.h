// The line descriptive layer for TRAINING with a backward (LineDescriptiveEncoder, models/line_transformer.py:75-91 of the reference =
// MultiHeadAttention + FeedForward, models/line_attention.py:23-94), in the project's folded form: only the CLS query
// row is computed, the key projection is folded into u_h = Wk_h^T (q_h / 8) and the value projection comes after the pooling.  What
// that leaves beside the exact-fp32 linear layers of lt_linbwd.h is here: three kernel families on float32 rows (row strides in floats,
// multiples of 4; 16-byte aligned bases; 16 bytes per lane and access).  The pooling's backward and the LayerNorm's forward and
// backward are each ONE body with two instances, without and with training-time dropout (template flag DROP; the dropout instances'
// kernels and the specification of their masks and arithmetic: lt_dropout.h), and each of their kernels is one call of its body.  The
// kernels' pointer parameters carry __restrict__, the bodies' do not (a second set of alias scopes only moves instructions).  Below,
// what the plain instances compute:
//
//   CLS token pooling, per segment l (S token rows of 256) and head h, u_lh [256]:
//     s_t = u_h . x_t     lse_h = log sum_t exp s_t     p_t = exp(s_t - lse_h)     pooled_h = sum_t p_t x_t
//     delta_h = dpooled_h . pooled_h (= sum_t p_t dp_t)     dp_t = dpooled_h . x_t     ds_t = p_t (dp_t - delta_h)
//     dx_t = sum_h (p_t dpooled_h + ds_t u_h)     du_h = sum_t ds_t x_t  (token order)
//   cp_fwd_kernel / cp_bwd_body: one wave per segment, lane i owns columns 4 i .. 4 i + 3 (a row is one coalesced 1 KB wave load), the
//   four heads' u (and dpooled) in registers, CP_TOK tokens in flight whose 4 x CP_TOK dot products are reduced together (wave_sum_n);
//   the forward's softmax is online over those chunks, so x comes from memory once per direction.  No LDS, no MFMA: bound by bytes.
//
//   LayerNorm over rows of 256 with an optional residual:  v = a + r (one float32 add)   mean, var two-pass on the row in registers
//     rstd = 1 / sqrt(var + eps)   y = (v - mean) rstd gamma + beta;   backward:  xhat = (v - mean) rstd   gg = fl(g gamma)
//     dx = rstd (gg - mean_c gg - xhat mean_c (gg xhat))   dgamma = sum_r g xhat   dbeta = sum_r g
//   ln_fwd_body / ln_bwd_body: one wave per row.  A block of the backward owns LN_CHUNK rows and writes one partial row of
//   dgamma | dbeta (float32: its waves' sums added in wave order); ln_reduce_kernel adds the chunks in ascending order in float64.
//
//   GELU, erf form:  y = z Phi(z)   dz = g (Phi(z) + z phi(z)),  Phi(z) = erfc(-z / sqrt 2) / 2 (no cancellation in the left tail),
//   phi(z) = exp(-z^2 / 2) / sqrt(2 pi);  gelu_kernel, four columns per thread, z kept by the caller for the backward.
//
// Deterministic: no atomics, every sum in a fixed order.  Every output element is written; nothing at or beyond the last row is
// loaded or stored.
#pragma once
#include "lt_common.h"

namespace lt {

constexpr int CP_SEGS = 4;         // segments (waves) per block of the pooling kernels
constexpr int CP_TOK = 4;          // forward: tokens in flight per wave (their 16 dot products are reduced together)
constexpr int CP_TOK_B = 2;        // backward: tokens in flight (2 x (4 scores + 4 dp) = 16 sums reduced together)
constexpr int CP_MAX_S = 256;
constexpr int LN_ROWS = 4;         // rows (waves) per block of the LayerNorm forward
constexpr int LN_CHUNK = 32;       // rows per block of the LayerNorm backward = per partial row of dgamma | dbeta

// (explicit fmas: one rounding sequence wherever it is inlined -- at S = 1 delta and dp are the same number, bit for bit, and ds = 0)
__device__ __forceinline__ float dot4(const f32x4 a, const f32x4 b) { return fmaf(a[3], b[3], fmaf(a[2], b[2], fmaf(a[1], b[1], a[0] * b[0]))); }

// ---- what the dropout instances draw their masks from (the generator and the counter layout: lt_dropout.h) ---------------------------

struct DropArgs {          // LinetrDropout as the kernels take it; a plain instance is handed an empty one and never reads it
  uint32_t key0, key1, call, threshold;
  float scale;
};

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

// ---- CLS token pooling -----------------------------------------------------------------------------------------------------------------

// (The forward is NOT a body with two instances: cp_drop_fwd_kernel of lt_dropout.h is a copy of this text with the factors added.  Both
// kernels compile to other instructions when their text is called through an inlined body, and the dropout one was then slower.)
// grid ceil(L / CP_SEGS), 256 threads.  x [L S][ldx], u [L][ldu >= 1024] -> pooled [L][1024], lse [L][4]
__global__ __launch_bounds__(256) void cp_fwd_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ u, int64_t ldu,
                                                     int64_t L, int S, float* __restrict__ pooled, float* __restrict__ lse) {
  const int lane = threadIdx.x & 63;
  const int64_t l = (int64_t)blockIdx.x * CP_SEGS + (threadIdx.x >> 6);
  if (l >= L) return;
  const int c = lane * 4;
  f32x4 uh[HEADS], acc[HEADS];
  float m[HEADS], den[HEADS];
#pragma unroll
  for (int h = 0; h < HEADS; ++h) {
    uh[h] = *reinterpret_cast<const f32x4*>(u + l * ldu + h * D + c);
    acc[h] = f32x4{0.f, 0.f, 0.f, 0.f};
    m[h] = -INFINITY;
    den[h] = 0.f;
  }
  const float* xs = x + l * S * ldx + c;
  for (int t0 = 0; t0 < S; t0 += CP_TOK) {
    f32x4 xv[CP_TOK];
    float s[CP_TOK * HEADS];
#pragma unroll
    for (int j = 0; j < CP_TOK; ++j)
      xv[j] = t0 + j < S ? *reinterpret_cast<const f32x4*>(xs + (int64_t)(t0 + j) * ldx) : f32x4{0.f, 0.f, 0.f, 0.f};
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
      float d = den[h] * scale;
      f32x4 a = acc[h] * scale;
#pragma unroll
      for (int j = 0; j < CP_TOK; ++j) {
        const float p = expf(s[j * HEADS + h] - mx);
        d += p;
        a += xv[j] * p;
      }
      m[h] = mx;
      den[h] = d;
      acc[h] = a;
    }
  }
#pragma unroll
  for (int h = 0; h < HEADS; ++h) {
    const float inv = 1.f / den[h];
    *reinterpret_cast<f32x4*>(pooled + l * (HEADS * D) + h * D + c) = acc[h] * inv;
  }
  if (lane < HEADS) {
    float v = 0.f;
#pragma unroll
    for (int h = 0; h < HEADS; ++h) v = lane == h ? m[h] + logf(den[h]) : v;
    lse[l * HEADS + lane] = v;
  }
}

// grid ceil(L / CP_SEGS), 256 threads.  dx [L S][lddx] and du [L][lddu]: each may be null.  DROP: site 0's factors generated again;
// dkept [L][4] may be null (no gradient arrives at kept)
template <bool DROP>
__device__ __forceinline__ void cp_bwd_body(const float* x, int64_t ldx, const float* u, int64_t ldu,
                                            const float* pooled, const float* lse, const float* kept,
                                            const float* dpooled, const float* dkept, int64_t L, int S,
                                            const DropArgs& dr, float* dx, int64_t lddx, float* du, int64_t lddu) {
  const int lane = threadIdx.x & 63;
  int64_t l = (int64_t)blockIdx.x * CP_SEGS;
  if constexpr (DROP) l += __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);       // (wave-uniform, provably: site 0's Philox calls run on the scalar unit)
  else l += threadIdx.x >> 6;
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
    if constexpr (DROP) dk[h] = dkept ? dkept[l * HEADS + h] : 0.f;
  }
  wave_sum_n(delta);
  if constexpr (DROP) {
    if (dkept) {
#pragma unroll
      for (int h = 0; h < HEADS; ++h) delta[h] = fmaf(dk[h], kept[l * HEADS + h], delta[h]);
    }
  }
  const float* xs = x + l * S * ldx + c;
  float* dxs = dx ? dx + l * S * lddx + c : nullptr;
  for (int t0 = 0; t0 < S; t0 += CP_TOK_B) {
    f32x4 xv[CP_TOK_B];
    float s[CP_TOK_B * 2 * HEADS], r[CP_TOK_B][HEADS];
#pragma unroll
    for (int j = 0; j < CP_TOK_B; ++j)
      xv[j] = t0 + j < S ? *reinterpret_cast<const f32x4*>(xs + (int64_t)(t0 + j) * ldx) : f32x4{0.f, 0.f, 0.f, 0.f};
    if constexpr (DROP) {
#pragma unroll
      for (int j = 0; j < CP_TOK_B; ++j) drop_factors(dr, 0u, (uint32_t)l, (uint32_t)(t0 + j), r[j]);
    }
#pragma unroll
    for (int j = 0; j < CP_TOK_B; ++j) {
      const f32x4 xp = DROP ? xv[j] * dr.scale : xv[j];     // a kept token as the forward pooled it: at S = 1 it IS pooled, bit for bit
#pragma unroll
      for (int h = 0; h < HEADS; ++h) {
        s[(j * 2) * HEADS + h] = dot4(uh[h], xv[j]);
        s[(j * 2 + 1) * HEADS + h] = dot4(dph[h], xp);
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
        float a = p, da = s[(j * 2 + 1) * HEADS + h];
        if constexpr (DROP) {
          a = p * r[j][h];
          // r da = scale (dpooled . x + dkept) for a kept token, rounded as delta is: at S = 1 both are the same number and ds = 0
          if (dkept) da = fmaf(dk[h], dr.scale, da);
          da = r[j][h] != 0.f ? da : 0.f;
        }
        const float ds = p * (da - delta[h]);
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

__global__ __launch_bounds__(256) void cp_bwd_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ u, int64_t ldu,
                                                     const float* __restrict__ pooled, const float* __restrict__ lse,
                                                     const float* __restrict__ dpooled, int64_t L, int S, float* __restrict__ dx,
                                                     int64_t lddx, float* __restrict__ du, int64_t lddu) {
  cp_bwd_body<false>(x, ldx, u, ldu, pooled, lse, nullptr, dpooled, nullptr, L, S, DropArgs{}, dx, lddx, du, lddu);
}

// ---- LayerNorm over rows of 256 ----------------------------------------------------------------------------------------------------

// One row of a wave: v = a + r, its mean and 1 / sqrt(var + eps), in passes over the row in registers; d <- v - mean.  The first mean
// m0 carries the rounding of a sum of 256 values; v - m0 is (nearly) exact where |mean| >> std, and the mean of those differences, a small
// number, corrects it: d = (v - m0) - corr keeps its digits at |mean| / std = 4096, where v - fl(mean) would be good to 2^-12 only.
__device__ __forceinline__ void ln_row_stats(const f32x4 v, float eps, f32x4& d, float& mean, float& rstd) {
  const float m0 = wave_sum((v[0] + v[1]) + (v[2] + v[3])) * (1.f / D);
  const f32x4 e = v - m0;
  const float corr = wave_sum((e[0] + e[1]) + (e[2] + e[3])) * (1.f / D);
  d = e - corr;
  mean = m0 + corr;
  const float var = wave_sum((d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3])) * (1.f / D);
  rstd = 1.f / sqrtf(var + eps);
}

// v = a + r of one lane's four columns of `row` (r may be null); DROP: v = fl(f a) + r, f <- the factors of `site` at (row, lane)
template <bool DROP>
__device__ __forceinline__ f32x4 ln_load_row(const float* a, int64_t lda, const float* r, int64_t ldr, int64_t row,
                                             int lane, const DropArgs& dr, uint32_t site, float (&f)[4]) {
  const int c = lane * 4;
  if constexpr (DROP) drop_factors(dr, site, (uint32_t)row, (uint32_t)lane, f);
  f32x4 v = *reinterpret_cast<const f32x4*>(a + row * lda + c);
  if constexpr (DROP) v = drop_apply(v, f);
  if (r) v += *reinterpret_cast<const f32x4*>(r + row * ldr + c);
  return v;
}

// grid ceil(rows / LN_ROWS), 256 threads.  r may be null.  stats [rows][2]: mean | rstd
template <bool DROP>
__device__ __forceinline__ void ln_fwd_body(const float* a, int64_t lda, const float* r, int64_t ldr,
                                            const float* gamma, const float* beta, float eps, int64_t rows,
                                            const DropArgs& dr, uint32_t site, float* y, int64_t ldy, float* stats) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * LN_ROWS + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int c = lane * 4;
  float f[4];
  const f32x4 v = ln_load_row<DROP>(a, lda, r, ldr, row, lane, dr, site, f);
  f32x4 d;
  float mean, rstd;
  ln_row_stats(v, eps, d, mean, rstd);
  const f32x4 gm = *reinterpret_cast<const f32x4*>(gamma + c), bt = *reinterpret_cast<const f32x4*>(beta + c);
  *reinterpret_cast<f32x4*>(y + row * ldy + c) = (d * rstd) * gm + bt;
  if (lane == 0) { stats[row * 2] = mean; stats[row * 2 + 1] = rstd; }
}

// grid ceil(rows / LN_CHUNK), 256 threads: wave w owns rows w, w + 4, .. of the chunk.  partial [gridDim.x][512]: dgamma | dbeta of the
// chunk (null: not wanted).  dres <- dv, the gradient of v (of a and of the residual alike without dropout); DROP: also da <- r dv.
// Each may be null.
template <bool DROP>
__device__ __forceinline__ void ln_bwd_body(const float* a, int64_t lda, const float* r, int64_t ldr,
                                            const float* stats, const float* gamma, const float* g,
                                            int64_t ldg, int64_t rows, const DropArgs& dr, uint32_t site, float* da, int64_t ldda,
                                            float* dres, int64_t lddr, float* partial) {
  __shared__ f32x4 red[3][2][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = lane * 4;
  const int64_t r0 = (int64_t)blockIdx.x * LN_CHUNK;
  const int64_t r1 = r0 + LN_CHUNK < rows ? r0 + LN_CHUNK : rows;
  const f32x4 gm = *reinterpret_cast<const f32x4*>(gamma + c);
  f32x4 dg = f32x4{0.f, 0.f, 0.f, 0.f}, db = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int64_t row = r0 + wave; row < r1; row += 4) {
    float f[4];
    const f32x4 v = ln_load_row<DROP>(a, lda, r, ldr, row, lane, dr, site, f);
    const f32x4 gv = *reinterpret_cast<const f32x4*>(g + row * ldg + c);
    const float mean = stats[row * 2], rstd = stats[row * 2 + 1];
    const f32x4 xh = (v - mean) * rstd;
    const f32x4 gg = mul_rounded(gv, gm);                  // (g gamma is rounded before the mean is subtracted)
    // every fma written out: one rounding sequence in both instances, whatever the compiler would contract
    float s[2] = {(gg[0] + gg[1]) + (gg[2] + gg[3]), fmaf(gg[0], xh[0], gg[1] * xh[1]) + fmaf(gg[2], xh[2], gg[3] * xh[3])};
    wave_sum_n(s);
    const float c1 = s[0] * (1.f / D), c2 = s[1] * (1.f / D);
    const f32x4 t = gg - c1;
    const f32x4 dv = f32x4{fmaf(-xh[0], c2, t[0]), fmaf(-xh[1], c2, t[1]), fmaf(-xh[2], c2, t[2]), fmaf(-xh[3], c2, t[3])} * rstd;
    if (dres) *reinterpret_cast<f32x4*>(dres + row * lddr + c) = dv;
    if constexpr (DROP) {
      if (da) *reinterpret_cast<f32x4*>(da + row * ldda + c) = drop_apply(dv, f);
    }
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

__global__ __launch_bounds__(256) void ln_fwd_kernel(const float* __restrict__ a, int64_t lda, const float* __restrict__ r, int64_t ldr,
                                                     const float* __restrict__ gamma, const float* __restrict__ beta, float eps, int64_t rows,
                                                     float* __restrict__ y, int64_t ldy, float* __restrict__ stats) {
  ln_fwd_body<false>(a, lda, r, ldr, gamma, beta, eps, rows, DropArgs{}, 0u, y, ldy, stats);
}

// (dx: the one data gradient, dv)
__global__ __launch_bounds__(256) void ln_bwd_kernel(const float* __restrict__ a, int64_t lda, const float* __restrict__ r, int64_t ldr,
                                                     const float* __restrict__ stats, const float* __restrict__ gamma,
                                                     const float* __restrict__ g, int64_t ldg, int64_t rows, float* __restrict__ dx,
                                                     int64_t lddx, float* __restrict__ partial) {
  ln_bwd_body<false>(a, lda, r, ldr, stats, gamma, g, ldg, rows, DropArgs{}, 0u, nullptr, 0, dx, lddx, partial);
}

// 512 threads in all: thread i adds column i of the partial rows in ascending chunk order, in float64
__global__ __launch_bounds__(256) void ln_reduce_kernel(const float* __restrict__ partial, int chunks, float* __restrict__ dgamma,
                                                        float* __restrict__ dbeta) {
  const int i = blockIdx.x * 256 + threadIdx.x;        // 0 .. 511
  double s = 0.0;
  for (int b = 0; b < chunks; ++b) s += (double)partial[(int64_t)b * (2 * D) + i];
  if (i < D) { if (dgamma) dgamma[i] = (float)s; }
  else if (dbeta) dbeta[i - D] = (float)s;
}

// ---- GELU, erf form ----------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ float gelu_cdf(float z) { return 0.5f * erfcf(z * -0.70710678118654752440f); }

// four columns per thread over rows x C / 4.  g null: y = gelu(z) -> out; else out = g gelu'(z)
__global__ __launch_bounds__(256) void gelu_kernel(const float* __restrict__ z, int64_t ldz, const float* __restrict__ g, int64_t ldg,
                                                   int64_t rows, int C, float* __restrict__ out, int64_t ldo) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int c4 = C / 4;
  if (i >= rows * c4) return;
  const int64_t row = i / c4;
  const int c = (int)(i - row * c4) * 4;
  const f32x4 zv = *reinterpret_cast<const f32x4*>(z + row * ldz + c);
  f32x4 o;
  if (g) {
    const f32x4 gv = *reinterpret_cast<const f32x4*>(g + row * ldg + c);
#pragma unroll
    for (int k = 0; k < 4; ++k)
      o[k] = gv[k] * (gelu_cdf(zv[k]) + zv[k] * (0.39894228040143267794f * expf(-0.5f * zv[k] * zv[k])));
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = zv[k] * gelu_cdf(zv[k]);
  }
  *reinterpret_cast<f32x4*>(out + row * ldo + c) = o;
}

}  // namespace lt
