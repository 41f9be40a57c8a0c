// Non-GEMM device stages of LineTransformer.forward (models/line_transformer.py:225-249): the first layers of the two positional
// encoders, mlp123_kernel, the CLS-row attention pooling and row_norm_kernel.  The signature attention is in lt_attn.h.
#pragma once
#include "lt_common.h"
#include "lt_token.h"
#include "lt_gemm_split.h"

namespace lt {

// ---------------------------------------------------------------------------------------------
// First MLP layer of the two positional encoders on the VALU (3 -> 32 and 5 -> 32, BN folded, ReLU),
// fused with normalize_keylines (models/line_transformer.py:22-38, :40-73).
// 8 threads per row, 4 output channels each.
// ---------------------------------------------------------------------------------------------
template <bool RELU = true>      // RELU = false: the pre-activations, for BatchNorm in training mode (lt_bntrain.h)
__global__ void word_mlp1_kernel(const float* __restrict__ pnt, const float* __restrict__ score, int64_t rows,
                                 float cx, float cy, float scale, const float* __restrict__ W /*[32][3]*/,
                                 const float* __restrict__ b, float* __restrict__ out /*[rows][32]*/) {
#pragma clang fp contract(off)
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t row = gid >> 3;
  if (row >= rows) return;
  const int c0 = (int)(gid & 7) * 4;
  const float x = (pnt[row * 2 + 0] - cx) / scale;
  const float y = (pnt[row * 2 + 1] - cy) / scale;
  const float s = score[row];
  f32x4 o;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const float* w = W + (c0 + c) * 3;
    float v = b[c0 + c] + w[0] * x + w[1] * y + w[2] * s;
    o[c] = RELU ? fmaxf(v, 0.f) : v;
  }
  *reinterpret_cast<f32x4*>(out + row * 32 + c0) = o;
}

template <bool RELU = true>
__global__ void line_mlp1_kernel(const float* __restrict__ sublines /*[N][2][2]*/, const float* __restrict__ resp,
                                 const float* __restrict__ angle, int N, float cx, float cy, float scale,
                                 const float* __restrict__ W /*[32][5]*/, const float* __restrict__ b,
                                 float* __restrict__ out /*[N][32]*/) {
#pragma clang fp contract(off)
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  const int row = gid >> 3;
  if (row >= N) return;
  const int c0 = (gid & 7) * 4;
  const float* sl = sublines + (int64_t)row * 4;
  const float sx = (sl[0] - cx) / scale, sy = (sl[1] - cy) / scale;
  const float ex = (sl[2] - cx) / scale, ey = (sl[3] - cy) / scale;
  const float in[5] = {(sx + ex) / 2.f, (sy + ey) / 2.f, resp[row], angle[row * 2], angle[row * 2 + 1]};
  f32x4 o;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const float* w = W + (c0 + c) * 5;
    float v = b[c0 + c];
#pragma unroll
    for (int i = 0; i < 5; ++i) v += w[i] * in[i];
    o[c] = RELU ? fmaxf(v, 0.f) : v;
  }
  *reinterpret_cast<f32x4*>(out + (int64_t)row * 32 + c0) = o;
}

// ---- layers 1-3 of a positional-encoder MLP in ONE pass (in -> 32 -> 64 -> 128, BN folded, ReLU) ---------------
// Exact-fp32 MFMA (v_mfma_f32_32x32x2_f32) on the TRANSPOSED product: neurons are the MFMA rows (A = weights,
// resident in VGPRs for the whole kernel), the 32 rows (tokens / sub-lines) of a step are the MFMA columns
// (B = activations).  The C/D layout -- lane = column, registers = rows (r&3) + 8(r>>2) + 4(lane>>5) -- is then
// exactly a B-operand layout of the next layer with the K index permuted, so bias + ReLU happen in registers and the
// activations never leave them: no LDS, no broadcasts (a v_readlane version spent 2/3 of its time in readlanes, a
// lane-per-row version with scalar-loaded weights thrashed the 16 KiB scalar cache).  Replaces mlp_first + the
// K = 32 and K = 64 GEMM launches (all prologue/epilogue at 9-30 TF) and keeps a1 / a2 out of HBM.
__device__ __forceinline__ void word_feat(const float* __restrict__ pnt, const float* __restrict__ score, int64_t row,
                                          float cx, float cy, float scale, float (&in)[3]) {
#pragma clang fp contract(off)
  in[0] = (pnt[row * 2 + 0] - cx) / scale;
  in[1] = (pnt[row * 2 + 1] - cy) / scale;
  in[2] = score[row];
}
__device__ __forceinline__ void line_feat(const float* __restrict__ sublines, const float* __restrict__ resp,
                                          const float* __restrict__ angle, int64_t row, float cx, float cy, float scale,
                                          float (&in)[5]) {
#pragma clang fp contract(off)
  const float* sl = sublines + row * 4;
  const float sx = (sl[0] - cx) / scale, sy = (sl[1] - cy) / scale;
  const float ex = (sl[2] - cx) / scale, ey = (sl[3] - cy) / scale;
  in[0] = (sx + ex) / 2.f; in[1] = (sy + ey) / 2.f; in[2] = resp[row]; in[3] = angle[row * 2]; in[4] = angle[row * 2 + 1];
}
// (the K index served by register r of an accumulator tile in lane half h is cd_row(r, h), lt_gemm.h; see above)

template <bool WORD>
__global__ __launch_bounds__(256) void mlp123_kernel(const float* __restrict__ p0, const float* __restrict__ p1,
                                                     const float* __restrict__ p2, int64_t rows, int rows_per_wave,
                                                     float cx, float cy, float scale,
                                                     const float* __restrict__ W1 /*[32][IN]*/, const float* __restrict__ b1,
                                                     const float* __restrict__ W2 /*[64][32]*/, const float* __restrict__ b2,
                                                     const float* __restrict__ W3 /*[128][64]*/, const float* __restrict__ b3,
                                                     float* __restrict__ out /*[rows][128]*/) {
  constexpr int IN = WORD ? 3 : 5;
  const int lane = threadIdx.x & 63, col = lane & 31, h = lane >> 5;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t r_begin = wave * rows_per_wave;
  const int64_t r_end = r_begin + rows_per_wave < rows ? r_begin + rows_per_wave : rows;
  // Stage W2 / W3 / biases in LDS once per block (coalesced float4 loads; row strides 33 / 65 floats so that the
  // per-lane gathers below are bank-conflict-free) -- per-lane gathers straight from global touch 32 lines per load.
  // LDS: the weight images are dead once every wave has gathered its registers; the per-wave output staging tiles
  // (32 rows x 68 floats each) reuse that space, which keeps the block at 43 KiB so that it can share a CU with the
  // blocks of a concurrent kernel (the NHWC transposition on the side stream) instead of waiting for them to drain.
  __shared__ __attribute__((aligned(16))) float sAll[64 * 33 + 128 * 65];
  __shared__ __attribute__((aligned(16))) float sW1[32 * 8];
  __shared__ __attribute__((aligned(16))) float sB[64 + 128];
  float* sW2 = sAll;
  float* sW3 = sAll + 64 * 33;
  float* stg = sAll + (threadIdx.x >> 6) * (32 * 68);
  static_assert(4 * 32 * 68 <= 64 * 33 + 128 * 65, "staging tiles must fit into the dead weight images");
  {  // all 10 loads of a thread are issued before the first LDS write (a load -> write loop pays the L2 latency 10x)
    f32x4 v2[2], v3[8];
#pragma unroll
    for (int u = 0; u < 2; ++u) v2[u] = *reinterpret_cast<const f32x4*>(W2 + (threadIdx.x + 256 * u) * 4);
#pragma unroll
    for (int u = 0; u < 8; ++u) v3[u] = *reinterpret_cast<const f32x4*>(W3 + (threadIdx.x + 256 * u) * 4);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int idx = threadIdx.x + 256 * u, r = idx / 8, c = (idx % 8) * 4;
#pragma unroll
      for (int q = 0; q < 4; ++q) sW2[r * 33 + c + q] = v2[u][q];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int idx = threadIdx.x + 256 * u, r = idx / 16, c = (idx % 16) * 4;
#pragma unroll
      for (int q = 0; q < 4; ++q) sW3[r * 65 + c + q] = v3[u][q];
    }
  }
  {  // layer-1 rows as [w0 .. w4, -, -, bias]
    const int k = threadIdx.x >> 3, c = threadIdx.x & 7;
    sW1[threadIdx.x] = c < IN ? W1[k * IN + c] : (c == 7 ? b1[k] : 0.f);
  }
  if (threadIdx.x < 64) sB[threadIdx.x] = b2[threadIdx.x];
  else if (threadIdx.x < 192) sB[threadIdx.x] = b3[threadIdx.x - 64];
  __syncthreads();
  // resident A operands.  Layer 2: K step s uses k = 2s + h (layer 1 is computed straight into that order).
  // Layer 3: K step (i, r) uses k = 32 i + cd_row(r, h), the order layer 2's accumulators come out in.
  float w2[2][16], w3[4][32];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int s2 = 0; s2 < 16; ++s2) w2[i][s2] = sW2[(32 * i + col) * 33 + 2 * s2 + h];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) w3[j][i * 16 + r] = sW3[(32 * j + col) * 65 + 32 * i + cd_row(r, h)];
  __syncthreads();                       // all waves hold their weights: sAll becomes the staging area
  if (r_begin >= r_end) return;
  float feat[IN], feat_next[IN];
  {
    int64_t row = r_begin + col;
    row = row < r_end ? row : r_end - 1;            // tail columns recompute the last row; their stores are masked
    if constexpr (WORD) word_feat(p0, p1, row, cx, cy, scale, feat);
    else line_feat(p0, p1, p2, row, cx, cy, scale, feat);
  }
  for (int64_t base = r_begin; base < r_end; base += 32) {
    {  // next step's inputs are requested now and consumed after this step's 160 MFMAs
      int64_t row = base + 32 + col;
      row = row < r_end ? row : r_end - 1;
      if constexpr (WORD) word_feat(p0, p1, row, cx, cy, scale, feat_next);
      else line_feat(p0, p1, p2, row, cx, cy, scale, feat_next);
    }
    // layer 1 on the VALU, rounded like word_mlp1_kernel / line_mlp1_kernel; this lane's neurons are k = 2s + h, their
    // weights come from LDS (kept as wave-uniform scalars they overflowed the SGPR file and were spilled lane by lane)
    float a1[16];
    {
#pragma clang fp contract(off)
#pragma unroll
      for (int s1 = 0; s1 < 16; ++s1) {
        const float* wr = sW1 + (2 * s1 + h) * 8;
        const f32x4 wa = *reinterpret_cast<const f32x4*>(wr), wb = *reinterpret_cast<const f32x4*>(wr + 4);
        const float wv[8] = {wa[0], wa[1], wa[2], wa[3], wb[0], wb[1], wb[2], wb[3]};
        float t = wv[7];                       // bias
#pragma unroll
        for (int i = 0; i < IN; ++i) t += wv[i] * feat[i];
        a1[s1] = fmaxf(t, 0.f);
      }
    }
    // layer 2: a2^T[64 neurons][32 rows] = W2 a1^T + b2.  The two 32-neuron tiles are interleaved: a chain of
    // dependent MFMAs on ONE accumulator runs at a fraction of the pipe rate (measured 4x slower per step).
    f32x16 acc2[2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 16; r += 4) {
        const f32x4 bv = *reinterpret_cast<const f32x4*>(sB + 32 * i + cd_row(r, h));
        acc2[i][r] = bv[0]; acc2[i][r + 1] = bv[1]; acc2[i][r + 2] = bv[2]; acc2[i][r + 3] = bv[3];
      }
#pragma unroll
    for (int s2 = 0; s2 < 16; ++s2)
#pragma unroll
      for (int i = 0; i < 2; ++i) acc2[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(w2[i][s2], a1[s2], acc2[i], 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc2[i][r] = fmaxf(acc2[i][r], 0.f);
    // layer 3, two 32-neuron tiles at a time (two independent accumulator chains); the 16 registers of a tile are
    // 4 runs of 4 consecutive neurons
#pragma unroll
    for (int jp = 0; jp < 2; ++jp) {
      f32x16 acc3[2];
#pragma unroll
      for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int r = 0; r < 16; r += 4) {
          const f32x4 bv = *reinterpret_cast<const f32x4*>(sB + 64 + 32 * (2 * jp + q) + cd_row(r, h));
          acc3[q][r] = bv[0]; acc3[q][r + 1] = bv[1]; acc3[q][r + 2] = bv[2]; acc3[q][r + 3] = bv[3];
        }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r)
#pragma unroll
          for (int q = 0; q < 2; ++q)
            acc3[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(w3[2 * jp + q][i * 16 + r], acc2[i][r], acc3[q], 0, 0, 0);
      // A lane owns one ROW in the accumulators, so storing from them would write 32-byte pieces 512 bytes apart.
      // Through this wave's staging tile ([32 rows][64 neurons of this pass], stride 68 floats) every store instruction
      // writes four complete 256-byte half rows.  LDS operations of one wave execute in order: no barrier needed.
#pragma unroll
      for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int r = 0; r < 16; r += 4)
          *reinterpret_cast<f32x4*>(stg + col * 68 + 32 * q + cd_row(r, h)) =
              f32x4{fmaxf(acc3[q][r], 0.f), fmaxf(acc3[q][r + 1], 0.f), fmaxf(acc3[q][r + 2], 0.f), fmaxf(acc3[q][r + 3], 0.f)};
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int t = 4 * i + (lane >> 4), pc = (lane & 15) * 4;
        if (base + t < r_end)
          *reinterpret_cast<f32x4*>(out + (base + t) * 128 + 64 * jp + pc) = *reinterpret_cast<const f32x4*>(stg + t * 68 + pc);
      }
      __builtin_amdgcn_wave_barrier();
    }
#pragma unroll
    for (int i = 0; i < IN; ++i) feat[i] = feat_next[i];
  }
}

// ---------------------------------------------------------------------------------------------
// CLS-row attention pooling of the line-descriptive layer (models/line_attention.py:6-75 restricted
// to query row 0, the only row that reaches the output: models/line_transformer.py:128).
//
// For head h the CLS query q_h is a model constant, so
//     score_hj = q_h . (Wk_h x_j + bk_h) = u_h . x_j + c_h ,   x_j = desc_j + W5 a4_j + b5
//              = u_h . desc_j + (W5^T u_h) . a4_j + const_h
// and the attention output only needs the attention-weighted means of desc_j and a4_j (the value and
// last-MLP projections are linear, they are applied after pooling by a [N x 544] x [544 x 64] GEMM).
// One 256-thread block per sub-line.
//   pooled[n][h] = [ sum_j p_hj desc_j (256) | sum_j p_hj a4_j (256) | p_h0 | 0 x31 ]
// ---------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void cls_pool_kernel(const float* __restrict__ desc /*[N][T][256]*/,
                                                       const float* __restrict__ a4 /*[N*T][256]*/, int T,
                                                       ClsPoolConst cc, float* __restrict__ pooled /*[N][4][544]*/) {
  extern __shared__ float sm[];  // [4][T+1]
  const int S = T + 1;
  const int n = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* dn = desc + (int64_t)n * T * D;
  const float* an = a4 + (int64_t)n * T * D;
  f32x4 u[4], u2[4];
#pragma unroll
  for (int h = 0; h < 4; ++h) {
    u[h] = *reinterpret_cast<const f32x4*>(cc.U + h * D + lane * 4);
    u2[h] = *reinterpret_cast<const f32x4*>(cc.U2 + h * D + lane * 4);
  }
  for (int j = wave; j < T; j += 4) {
    const f32x4 dv = *reinterpret_cast<const f32x4*>(dn + j * D + lane * 4);
    const f32x4 av = *reinterpret_cast<const f32x4*>(an + j * D + lane * 4);
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      float p = 0.f;
#pragma unroll
      for (int c = 0; c < 4; ++c) p += dv[c] * u[h][c] + av[c] * u2[h][c];
      p = wave_sum(p);
      if (lane == 0) sm[h * S + 1 + j] = p + cc.c_tok[h];
    }
  }
  if (tid < 4) sm[tid * S] = cc.s_cls[tid];
  __syncthreads();
  if (tid < 4) {  // softmax over the S keys of head `tid` (F.softmax, line_attention.py:18)
    float* s = sm + tid * S;
    float mx = s[0];
    for (int j = 1; j < S; ++j) mx = fmaxf(mx, s[j]);
    float sum = 0.f;
    for (int j = 0; j < S; ++j) { s[j] = expf(s[j] - mx); sum += s[j]; }
    for (int j = 0; j < S; ++j) s[j] = s[j] / sum;
  }
  __syncthreads();
  float db[4] = {0.f, 0.f, 0.f, 0.f}, ab[4] = {0.f, 0.f, 0.f, 0.f};
  for (int j = 0; j < T; ++j) {
    const float dv = dn[j * D + tid], av = an[j * D + tid];
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      const float p = sm[h * S + 1 + j];
      db[h] += p * dv;
      ab[h] += p * av;
    }
  }
  float* out = pooled + (int64_t)n * 4 * POOLW;
#pragma unroll
  for (int h = 0; h < 4; ++h) {
    out[h * POOLW + tid] = db[h];
    out[h * POOLW + 256 + tid] = ab[h];
  }
  if (tid < 4 * 32) {
    const int h = tid >> 5, i = tid & 31;
    out[h * POOLW + 512 + i] = i == 0 ? sm[h * S] : 0.f;
  }
}

// ---------------------------------------------------------------------------------------------
// Pooling for the batched fast path (linetr_describe): same mathematics as cls_pool_kernel up to fp32 rounding, but
//   * token descriptors are sampled from the NHWC map on the fly -- the [N,T,256] tensor of the reference is never
//     materialised;
//   * only REAL tokens are visited; every zero-padding slot of an image holds the same coordinate (0,0)
//     (models/line_process.py:133-139), i.e. identical descriptor / a4 row / score, so the padding slots
//     enter the softmax as ONE key with multiplicity n_pad.
// a4 / cpnt are indexed by the compact token list (rec.first_tok), the image's padding token sits at first_pad + image.
// ONE WAVE PER SUB-LINE (4 per block), online softmax (running max / sum per head, rescaled accumulators) so every
// token is visited once, nothing is staged in LDS and there is no barrier; the bilinear taps and the a4 row of token
// j+1 are in flight while token j is reduced.  The softmax normalisation is applied at the end.
// ---------------------------------------------------------------------------------------------
// SPLIT = 4 (a few hundred sub-lines: a single pair): the block's four waves share ONE sub-line, wave w taking tokens w, w + 4, ..;
// the four partial (max, sum, pooled sums) states are merged through LDS, wave h finishing head h.  The dependent chain per wave is a
// quarter as long (21 tokens -> 6): 24 -> 10 us at cfg2.
// The kernel's text is lt_cls_pool_online_body.h, included once per geometry.  All images of one size: their channel-last maps lie back to
// back, image i at i * Hc * Wc * 256 floats.
#define LT_POOL_KERNEL cls_pool_online_kernel
#define LT_POOL_TPARAMS
#define LT_POOL_MAP_PARAMS const float* __restrict__ nhwc, int Hc, int Wc
#define LT_POOL_MAP(image) typedef float PoolElem; const float* nhwc_img = nhwc + (int64_t)image * Hc * Wc * D;
#include "lt_cls_pool_online_body.h"
#undef LT_POOL_KERNEL
#undef LT_POOL_TPARAMS
#undef LT_POOL_MAP_PARAMS
#undef LT_POOL_MAP

// the same on a half map (E = f16_t or bf16_t): 8 bytes per lane and tap, widened where the tap set is first used
#define LT_POOL_KERNEL cls_pool_online_typed_kernel
#define LT_POOL_TPARAMS , class E
#define LT_POOL_MAP_PARAMS const E* __restrict__ nhwc, int Hc, int Wc
#define LT_POOL_MAP(image) typedef E PoolElem; const E* nhwc_img = nhwc + (int64_t)image * Hc * Wc * D;
#include "lt_cls_pool_online_body.h"
#undef LT_POOL_KERNEL
#undef LT_POOL_TPARAMS
#undef LT_POOL_MAP_PARAMS
#undef LT_POOL_MAP

// ragged (linetr_describe_ragged): the sub-line's image has its own map and size in the image table.  The entry is wave-uniform (a wave
// works on one sub-line): it is loaded once per wave, through the scalar unit.
#define LT_POOL_KERNEL cls_pool_online_ragged_kernel
#define LT_POOL_TPARAMS
#define LT_POOL_MAP_PARAMS const RaggedImage* __restrict__ tab
#define LT_POOL_MAP(image)                                                  \
  typedef float PoolElem;                                                   \
  const RaggedImage& im_ = tab[__builtin_amdgcn_readfirstlane(image)];      \
  const float* nhwc_img = (const float*)im_.nhwc;                           \
  const int Hc = im_.Hc, Wc = im_.Wc;
#include "lt_cls_pool_online_body.h"
#undef LT_POOL_KERNEL
#undef LT_POOL_TPARAMS
#undef LT_POOL_MAP_PARAMS
#undef LT_POOL_MAP

#define LT_POOL_KERNEL cls_pool_online_ragged_typed_kernel
#define LT_POOL_TPARAMS , class E
#define LT_POOL_MAP_PARAMS const RaggedImage* __restrict__ tab
#define LT_POOL_MAP(image)                                                  \
  typedef E PoolElem;                                                       \
  const RaggedImage& im_ = tab[__builtin_amdgcn_readfirstlane(image)];      \
  const E* nhwc_img = (const E*)im_.nhwc;                                   \
  const int Hc = im_.Hc, Wc = im_.Wc;
#include "lt_cls_pool_online_body.h"
#undef LT_POOL_KERNEL
#undef LT_POOL_TPARAMS
#undef LT_POOL_MAP_PARAMS
#undef LT_POOL_MAP

// ---------------------------------------------------------------------------------------------
// Row kernels over [rows][256]; one wave64 per row, lane = 4 channels.
//   mode 0: y = LayerNorm(x) * gamma + beta (+ add)      eps = 1e-6 (models/line_attention.py:40,83)
//   mode 1: y = x / max(||x||_2, 1e-12) (+ add)          F.normalize (models/line_transformer.py:246)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void row_norm_kernel(const float* __restrict__ x, int rows, int mode,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       const float* __restrict__ add, float eps, float* __restrict__ y) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  f32x4 v = *reinterpret_cast<const f32x4*>(x + (int64_t)row * D + lane * 4);
  f32x4 o;
  if (mode == 0) {
    float mean = wave_sum(v[0] + v[1] + v[2] + v[3]) * (1.f / D);
    float q = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) { float d = v[c] - mean; q += d * d; }
    const float rstd = 1.f / sqrtf(wave_sum(q) * (1.f / D) + eps);
    const f32x4 g = *reinterpret_cast<const f32x4*>(gamma + lane * 4);
    const f32x4 b = *reinterpret_cast<const f32x4*>(beta + lane * 4);
#pragma unroll
    for (int c = 0; c < 4; ++c) o[c] = (v[c] - mean) * rstd * g[c] + b[c];
  } else {
    float q = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) q += v[c] * v[c];
    const float nrm = fmaxf(sqrtf(wave_sum(q)), 1e-12f);
#pragma unroll
    for (int c = 0; c < 4; ++c) o[c] = v[c] / nrm;
  }
  if (add) {      // behind either normalisation, as the fused epilogue of lt_gemm_split.h does (GemmArgs::add2)
    const f32x4 a = *reinterpret_cast<const f32x4*>(add + (int64_t)row * D + lane * 4);
#pragma unroll
    for (int c = 0; c < 4; ++c) o[c] += a[c];
  }
  *reinterpret_cast<f32x4*>(y + (int64_t)row * D + lane * 4) = o;
}

}  // namespace lt
