// SuperPoint's shared encoder and the two head convolutions (models/superpoint.py:113-127, 148-160, 188-189), inference only,
// channel-last inside:
//   sp_conv1a_kernel   conv1a, Cin = 1: nine taps are no GEMM -- a direct vector kernel, gray image [B,1,H,W] -> [B,H,W,64]
//   sp_conv_kernel     every other layer as an implicit GEMM on exact-fp32 MFMA (v_mfma_f32_32x32x2_f32, fp32 accumulation):
//                      M = the pixels of an 8 x 16 spatial tile, N = output channels, K = (input-channel chunk, tap, channel).
//                      KS = 3: 3x3 / stride 1 / zero padding 1 + bias + ReLU, with POOL followed by the 2x2 / stride 2 maximum
//                      in the epilogue (the pre-pool map never reaches memory).  KS = 1: the 1x1 head layers convPb / convDb on
//                      the [cells, 512] rows the fused convPa | convDa launch wrote -- the same body with one tap and no halo.
//   sp_pack_kernel     state_dict weights [Cout, Cin, KS, KS] -> the K order the kernel walks (once per weight set)
//
// CDNA4 mapping of sp_conv_kernel
//   * 256 threads = 4 wave64 as 2 x 2: wave (wm, wn) owns 64 pixels (tile rows 4 wm .. 4 wm + 3) x COUT_TILE / 2 channels,
//     i.e. 2 x NI accumulators of 32 x 32.
//   * The block stages the (TH + 2) x (TW + 2) halo patch of its tile in LDS, 32 input channels at a time, as [position][32 + 4]:
//     the row stride of 36 dwords is the GEMM family's (lt_gemm.h) and keeps ds_read_b128 of a 16-lane group on distinct banks.
//     Positions outside the image are zero-filled; the nine taps are nine shifted views of the one patch, so an input element is
//     fetched once per block and chunk, not nine times.
//   * K-permutation of lt_gemm.h: one 128-bit read gives a lane 4 consecutive channels of its pixel; MFMA step s of 8-channel group kk
//     consumes element s of both wave halves, i.e. channel 8 kk + 4 (lane >> 5) + s.  The packed weights use the same mapping:
//       packed[((chunk * KS * KS + tap) * 4 + kk) * Cout + n][8]  =  w[n][32 chunk + 8 kk + 0..7][tap]
//     so a wave's B-operand load (32 channels n x two halves of 16 bytes) is 1 KiB contiguous.  Weights go global -> registers (at most
//     1.2 MB per layer, L2-resident), one tap ahead of the MFMAs that consume them.
//   * C/D layout (cd_row): register r of lane (n = lane & 31, half h) is tile pixel (r & 3) + 8 (r >> 2) + 4 h of its 32-pixel group =
//     two tile rows of 16.  The four pixels of a 2x2 pooling window are registers r, r + 1, r + 8, r + 9 of ONE lane (r = 0, 2, 4, 6),
//     so the pool is lane-local.  Tiles start at even coordinates; pooling floors like nn.MaxPool2d(2, 2): an odd last row or column
//     is computed and dropped.
//   * No atomics; rows, columns and channels beyond the tensor are neither loaded nor stored; a result is a fixed sum order, so the
//     same call gives the same bits.
#pragma once
#include "lt_common.h"
#include "lt_gemm.h"

namespace lt {

constexpr int SP_TH = 8, SP_TW = 16;       // spatial tile of sp_conv_kernel (pixels; both even: pooling windows never straddle tiles)
constexpr int SP_CK = 32;                  // input channels staged per chunk
constexpr int SP_LS = GEMM_LDS_STRIDE;     // floats per staged position

struct SpConvArgs {
  const float* x; int64_t ldx;     // input pixels [B, H, W] of ldx floats each; the layer reads channels 0 .. CIN - 1 of a pixel
  const float* w;                  // packed weights (sp_pack_kernel), cout_packed output channels
  const float* bias;               // [cout_packed]
  float* y; int64_t ldy;           // output pixels [B, Ho, Wo] of ldy floats each (Ho = H / 2 with POOL)
  int H, W;
  int cout_packed;                 // multiple of COUT_TILE
  int cout_store;                  // channels n >= cout_store are padding: computed, never stored
  int relu;
};

// offset (floats) of w[n][c][tap] in the packed weight of a layer with Cout = cout_packed
__host__ __device__ inline int64_t sp_pack_index(int n, int c, int tap, int taps, int cout_packed) {
  const int chunk = c / SP_CK, kk = (c % SP_CK) / 8, e = c % 8;
  return ((((int64_t)chunk * taps + tap) * 4 + kk) * cout_packed + n) * 8 + e;
}

// src [cout_src][cin][taps] (state_dict layout, tap = ky * KS + kx) -> rows cout_off .. cout_off + cout_src - 1 of the packed weight
__global__ __launch_bounds__(256) void sp_pack_kernel(const float* __restrict__ src, int cout_src, int cin, int taps,
                                                      float* __restrict__ dst, int cout_packed, int cout_off) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)cout_src * cin * taps) return;
  const int tap = (int)(i % taps), c = (int)((i / taps) % cin), n = (int)(i / ((int64_t)taps * cin));
  dst[sp_pack_index(cout_off + n, c, tap, taps, cout_packed)] = src[i];
}

template <int CIN, int COUT_TILE, int KS, bool POOL>
__global__ __launch_bounds__(256) void sp_conv_kernel(SpConvArgs a) {
  static_assert(CIN % SP_CK == 0 && (COUT_TILE == 64 || COUT_TILE == 128) && (KS == 1 || KS == 3) && !(POOL && KS == 1), "unsupported layer");
  constexpr int PAD = KS / 2, PH = SP_TH + 2 * PAD, PW = SP_TW + 2 * PAD, TAPS = KS * KS;
  constexpr int NI = COUT_TILE / 64;       // 32-channel accumulators per wave
  constexpr int NCHUNK = CIN / SP_CK;
  constexpr int LS = SP_LS;
  __shared__ __attribute__((aligned(16))) float patch[PH * PW * LS];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, half = lane >> 5;
  const int tiles_x = (a.W + SP_TW - 1) / SP_TW;
  const int y0 = (int)(blockIdx.x / tiles_x) * SP_TH, x0 = (int)(blockIdx.x % tiles_x) * SP_TW;
  const int n0 = blockIdx.y * COUT_TILE + wn * (COUT_TILE / 2);
  const int b = blockIdx.z;
  const float* xb = a.x + (int64_t)b * a.H * a.W * a.ldx;

  f32x16 acc[2][NI];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // A operand: accumulator i of this wave covers tile rows 4 wm + 2 i, + 1; the lane's pixel is row (lane & 31) >> 4, column lane & 15
  const int apos = ((4 * wm + ((lane & 31) >> 4)) * PW + (lane & 15)) * LS + 4 * half;
  // B operand: 16 bytes at channel n0 + 32 j + (lane & 31), half `half` of an 8-channel group
  const float* wl = a.w + ((int64_t)n0 + (lane & 31)) * 8 + 4 * half;
  const int64_t wstep = (int64_t)a.cout_packed * 8;       // one 8-channel group

  f32x4 bw[2][4][NI];
  auto wload = [&](int buf, int kg0) {
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
#pragma unroll
      for (int j = 0; j < NI; ++j) bw[buf][kk][j] = *reinterpret_cast<const f32x4*>(wl + (kg0 + kk) * wstep + j * 32 * 8);
  };

  for (int chunk = 0; chunk < NCHUNK; ++chunk) {
    if (chunk) __syncthreads();            // everyone has finished reading the previous chunk's patch
    for (int i = tid; i < PH * PW * (SP_CK / 4); i += 256) {
      const int pos = i / (SP_CK / 4), q = i % (SP_CK / 4);
      const int gy = y0 - PAD + pos / PW, gx = x0 - PAD + pos % PW;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (gy >= 0 && gy < a.H && gx >= 0 && gx < a.W)
        v = *reinterpret_cast<const f32x4*>(xb + ((int64_t)gy * a.W + gx) * a.ldx + chunk * SP_CK + 4 * q);
      *reinterpret_cast<f32x4*>(&patch[pos * LS + 4 * q]) = v;
    }
    wload(0, chunk * TAPS * 4);
    __syncthreads();
#pragma unroll
    for (int tap = 0; tap < TAPS; ++tap) {
      const int cur = tap & 1;
      if (tap + 1 < TAPS) wload(cur ^ 1, (chunk * TAPS + tap + 1) * 4);
      const float* ap = patch + apos + ((tap / KS) * PW + tap % KS) * LS;
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        f32x4 af[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) af[i] = *reinterpret_cast<const f32x4*>(ap + i * 2 * PW * LS + kk * 8);
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
          for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < NI; ++j)
              acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i][s], bw[cur][kk][j][s], acc[i][j], 0, 0, 0);
      }
    }
  }

  // epilogue: bias, ReLU, optional lane-local 2x2 maximum, store
  const int Ho = POOL ? a.H / 2 : a.H, Wo = POOL ? a.W / 2 : a.W;
  float* yb = a.y + (int64_t)b * Ho * Wo * a.ldy;
#pragma unroll
  for (int j = 0; j < NI; ++j) {
    const int n = n0 + j * 32 + (lane & 31);
    const float bv = a.bias[n];
    const bool n_ok = n < a.cout_store;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      float v[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        v[r] = acc[i][j][r] + bv;
        if (a.relu) v[r] = fmaxf(v[r], 0.f);
      }
      if constexpr (POOL) {
        const int oy = (y0 >> 1) + 2 * wm + i;
#pragma unroll
        for (int r = 0; r < 8; r += 2) {
          const int ox = (x0 >> 1) + (((r & 3) + 8 * (r >> 2) + 4 * half) >> 1);
          if (n_ok && oy < Ho && ox < Wo)
            yb[((int64_t)oy * Wo + ox) * a.ldy + n] = fmaxf(fmaxf(v[r], v[r + 1]), fmaxf(v[r + 8], v[r + 9]));
        }
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int p = cd_row(r, half);                       // pixel of the 32-pixel group: two tile rows of 16
          const int oy = y0 + 4 * wm + 2 * i + (p >> 4), ox = x0 + (p & 15);
          if (n_ok && oy < Ho && ox < Wo) yb[((int64_t)oy * Wo + ox) * a.ldy + n] = v[r];
        }
      }
    }
  }
}

// conv1a: one thread = one pixel x 4 output channels (16 threads per pixel write its 256 bytes contiguously).
// w [64][9] and bias [64] in state_dict layout; taps outside the image contribute nothing (zero padding).
__global__ __launch_bounds__(256) void sp_conv1a_kernel(const float* __restrict__ img, const float* __restrict__ w,
                                                        const float* __restrict__ bias, float* __restrict__ y, int H, int W,
                                                        int64_t pixels) {
  const int64_t p = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
  if (p >= pixels) return;
  const int q = threadIdx.x & 15;
  const int px = (int)(p % W), py = (int)((p / W) % H);
  const float* row = img + (p - px - (int64_t)py * W);          // the pixel's image
  float in[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    const int gy = py + t / 3 - 1, gx = px + t % 3 - 1;
    in[t] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? row[(int64_t)gy * W + gx] : 0.f;
  }
  f32x4 o;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const float* wc = w + (4 * q + c) * 9;
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < 9; ++t) s = fmaf(in[t], wc[t], s);
    o[c] = fmaxf(s + bias[4 * q + c], 0.f);
  }
  *reinterpret_cast<f32x4*>(y + p * 64 + 4 * q) = o;
}

}  // namespace lt
