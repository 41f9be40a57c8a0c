// The two kernels of the SuperPoint head producer (lt_producer.h has their description), as text that lt_producer.h includes once per
// family of element types: no include guard.  The float32 kernels keep the names, signatures and text they always had, so that they compile
// to the same code (sharing the text through an inlined function template moved the FMA contraction of the descriptor kernel's squared
// norm, and with it the last bits of what float32 callers get).  The including file defines
//   LT_HEAD_DESC_TEMPLATE / LT_HEAD_DESC_KERNEL     template header and name of the descriptor kernel
//   LT_HEAD_SCORE_TEMPLATE / LT_HEAD_SCORE_KERNEL   the same for the score kernel
//   LT_HEAD_EI / LT_HEAD_EO                         element types of the raw inputs and of the two descriptor outputs, as parameter types
//   LT_HEAD_LD_PARAM                                `, int64_t ld` where the kernel takes a row stride
//   LT_HEAD_DESC_PROLOGUE / LT_HEAD_SCORE_PROLOGUE  statements that define EI (descriptor kernel: and EO) and, where they are no
//                                                   parameters, ROWS and ld
// A half input is widened at the load (exact), a half output rounded at the store (nearest-even); the tile, the norm and the products are
// float32 whatever the types, so half outputs are the float32 outputs rounded.  The 4-cell vector path of a half side is 8 bytes per lane.
LT_HEAD_DESC_TEMPLATE
__global__ __launch_bounds__(256) void LT_HEAD_DESC_KERNEL(const LT_HEAD_EI* __restrict__ raw, LT_HEAD_EO* __restrict__ nhwc,
                                                           LT_HEAD_EO* __restrict__ nchw, int HW LT_HEAD_LD_PARAM) {
  LT_HEAD_DESC_PROLOGUE
  constexpr bool F32_OUT = sizeof(EO) == 4;
  constexpr int LS = CELLS + 1;
  constexpr int LPC = CELLS / 4;          // lanes per channel row (one float4 each)
  constexpr int CPP = 256 / LPC;          // channels per pass
  constexpr int NG = 256 / CELLS;         // partial sums per cell
  __shared__ float tile[D * LS];
  __shared__ float part[256];
  const int t = threadIdx.x, b = blockIdx.y, p0 = blockIdx.x * CELLS;
  const EI* src = raw + (int64_t)b * D * HW;
  const bool vec = (HW % 4) == 0;
  const int cl = t / LPC, p4 = (t % LPC) * 4;
  // phase 1: CPP channels per pass, LPC lanes x 4 cells per channel (rows: one wave per cell, 256 B per instruction)
  if constexpr (ROWS) {
    const int lane = t & 63, w = t >> 6;
    for (int p = w; p < CELLS; p += 4) {
      const bool in = p0 + p < HW;
      const EI* s = raw + ((int64_t)b * HW + p0 + p) * ld;
#pragma unroll
      for (int i = 0; i < 4; ++i) tile[(lane + 64 * i) * LS + p] = in ? Elem<EI>::widen(s[lane + 64 * i]) : 0.f;
    }
  } else
#pragma unroll 4
  for (int pass = 0; pass < D / CPP; ++pass) {
    const int c = pass * CPP + cl;
    const EI* s = src + (int64_t)c * HW + p0 + p4;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (vec && p0 + p4 + 3 < HW) v = Elem<EI>::widen(load_raw4(s));
    else {
#pragma unroll
      for (int j = 0; j < 4; ++j) if (p0 + p4 + j < HW) v[j] = Elem<EI>::widen(s[j]);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) tile[c * LS + p4 + j] = v[j];
  }
  __syncthreads();
  // phase 2: squared norm of every cell over the 256 channels (NG partial sums of D / NG channels)
  {
    const int p = t % CELLS, g = t / CELLS;
    float ss = 0.f;
#pragma unroll 8
    for (int c = g * (D / NG); c < (g + 1) * (D / NG); ++c) { const float v = tile[c * LS + p]; ss += v * v; }
    part[g * CELLS + p] = ss;
  }
  __syncthreads();
  if (t < CELLS) {
    float ss = 0.f;
#pragma unroll
    for (int g = 0; g < NG; ++g) ss += part[g * CELLS + t];
    part[t] = 1.f / fmaxf(sqrtf(ss), 1e-12f);   // F.normalize: x / max(||x||, eps)   (part[t] is only read by t above)
  }
  __syncthreads();
  // phase 3a: NHWC, one cell = 1 KiB contiguous; a wave writes 256 B per instruction
  if (nhwc) {
    const int lane = t & 63, w = t >> 6;
    EO* dst = nhwc + ((int64_t)b * HW + p0) * D;
    for (int p = w; p < CELLS; p += 4) {
      if (p0 + p >= HW) break;
      const float inv = part[p];
      if constexpr (F32_OUT) {
#pragma unroll
        for (int i = 0; i < 4; ++i) dst[(int64_t)p * D + lane + 64 * i] = tile[(lane + 64 * i) * LS + p] * inv;
      } else {   // a lane owns two neighbouring channels, 4 bytes: the wave still writes 256 B per instruction.  (Channel rows are 33 dwords
        // apart, so these reads are 2-way bank-conflicted; a mapping without the conflict -- lanes 16-31 of each half reading their odd
        // channel first -- measured the same, 0.239 against 0.234 ms for 128 images: the kernel does not wait for LDS.)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const int c = 2 * lane + 128 * i;
          struct alignas(4) Pair { EO a, b; };
          *reinterpret_cast<Pair*>(dst + (int64_t)p * D + c) =
              Pair{Elem<EO>::narrow(tile[c * LS + p] * inv), Elem<EO>::narrow(tile[(c + 1) * LS + p] * inv)};
        }
      }
    }
  }
  // phase 3b: normalised NCHW (the reference's 'dense_descriptor' key), same access pattern as phase 1
  if (nchw) {
    EO* dstb = nchw + (int64_t)b * D * HW;
#pragma unroll 4
    for (int pass = 0; pass < D / CPP; ++pass) {
      const int c = pass * CPP + cl;
      EO* d = dstb + (int64_t)c * HW + p0 + p4;
      f32x4 v;
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = tile[c * LS + p4 + j] * part[p4 + j];
      if constexpr (F32_OUT) {
        if (vec && p0 + p4 + 3 < HW) *reinterpret_cast<f32x4*>(d) = v;
        else {
#pragma unroll
          for (int j = 0; j < 4; ++j) if (p0 + p4 + j < HW) d[j] = v[j];
        }
      } else {
        struct alignas(8) Quad { EO e[4]; };
        if (vec && p0 + p4 + 3 < HW)
          *reinterpret_cast<Quad*>(d) = Quad{{Elem<EO>::narrow(v[0]), Elem<EO>::narrow(v[1]), Elem<EO>::narrow(v[2]), Elem<EO>::narrow(v[3])}};
        else {
#pragma unroll
          for (int j = 0; j < 4; ++j) if (p0 + p4 + j < HW) d[j] = Elem<EO>::narrow(v[j]);
        }
      }
    }
  }
}

// One block = 64 consecutive cells of one image x 65 logits.  Thread (cell p, quarter g) owns the 16 channels of
// sub-pixel rows dy = 2g, 2g+1 of its cell's 8x8 patch (quarter 3 also the dustbin): one expf per output, the
// max and the sum are combined across the four quarters through LDS.
// ROWS: logits are channel-last rows [B * HW][ld >= 65] instead of NCHW (as for sp_desc_head_kernel: the load alone differs).
LT_HEAD_SCORE_TEMPLATE
__global__ __launch_bounds__(256) void LT_HEAD_SCORE_KERNEL(const LT_HEAD_EI* __restrict__ logits, float* __restrict__ score,
                                                            int Hc, int Wc LT_HEAD_LD_PARAM) {
  LT_HEAD_SCORE_PROLOGUE
  constexpr int LS = 65;
  __shared__ float tile[65 * LS];
  __shared__ float red[2][4 * 64];
  const int t = threadIdx.x, b = blockIdx.y, p0 = blockIdx.x * 64, HW = Hc * Wc;
  const EI* src = logits + (int64_t)b * 65 * HW;
  const bool vec = (HW % 4) == 0;
  if constexpr (ROWS) {
    for (int i = t; i < 64 * 65; i += 256) {
      const int p = i / 65, c = i % 65;
      tile[c * LS + p] = p0 + p < HW ? Elem<EI>::widen(logits[((int64_t)b * HW + p0 + p) * ld + c]) : 0.f;
    }
  } else {  // 16 lanes x 4 cells per channel row, 16 channels per pass (+ the dustbin row)
    const int cl = t >> 4, p4 = (t & 15) * 4;
#pragma unroll
    for (int pass = 0; pass < 5; ++pass) {
      const int c = pass * 16 + cl;
      if (c < 65) {
        const EI* sp = src + (int64_t)c * HW + p0 + p4;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (vec && p0 + p4 + 3 < HW) v = Elem<EI>::widen(load_raw4(sp));
        else {
#pragma unroll
          for (int j = 0; j < 4; ++j) if (p0 + p4 + j < HW) v[j] = Elem<EI>::widen(sp[j]);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) tile[c * LS + p4 + j] = v[j];
      }
    }
  }
  __syncthreads();
  const int p = t & 63, g = t >> 6;
  float x[17];
#pragma unroll
  for (int i = 0; i < 16; ++i) x[i] = tile[(g * 16 + i) * LS + p];
  x[16] = g == 3 ? tile[64 * LS + p] : -INFINITY;
  float m = x[0];
#pragma unroll
  for (int i = 1; i < 17; ++i) m = fmaxf(m, x[i]);
  red[0][g * 64 + p] = m;
  __syncthreads();
  m = fmaxf(fmaxf(red[0][p], red[0][64 + p]), fmaxf(red[0][128 + p], red[0][192 + p]));
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < 17; ++i) { x[i] = expf(x[i] - m); sum += x[i]; }   // expf(-inf) = 0 for the missing dustbin slots
  red[1][g * 64 + p] = sum;
  __syncthreads();
  if (p0 + p >= HW) return;
  const float inv = 1.f / ((red[1][p] + red[1][64 + p]) + (red[1][128 + p] + red[1][192 + p]));
  const int cell = p0 + p, hh = cell / Wc, ww = cell % Wc;
  const int W8 = Wc * 8;
  float* dst = score + (int64_t)b * (Hc * 8) * W8 + (int64_t)(hh * 8) * W8 + ww * 8;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    float* d = dst + (int64_t)(2 * g + r) * W8;     // 8 * ww floats into a row of 8 * Wc: always 16-byte aligned
    *reinterpret_cast<f32x4*>(d) = f32x4{x[r * 8 + 0] * inv, x[r * 8 + 1] * inv, x[r * 8 + 2] * inv, x[r * 8 + 3] * inv};
    *reinterpret_cast<f32x4*>(d + 4) = f32x4{x[r * 8 + 4] * inv, x[r * 8 + 5] * inv, x[r * 8 + 6] * inv, x[r * 8 + 7] * inv};
  }
}
