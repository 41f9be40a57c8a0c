// Fixed-size training samples on the device: the 'klines' branch of the reference's conv_fixed_size
// (dataloaders/utils/util_lines.py:695-766) for a batch.  Image b's tokeniser tensors are padded to max_sublines (M) rows with tokenised
// pseudo lines, or cut to M rows, and written straight to row b * M + j of the [B, M, ...] outputs: no var-len intermediate, every
// output byte stored once.  The rows themselves are the tokeniser's (tokenize_subline / kline_row / sample_one of lt_token.h, one body
// each); what is new here is the index work:
//   - the row map.  Row j of image b is sub-line j of the image while j < min(num_slns, M) -- its key-line is found by a binary search
//     of the image's records, whose first_sub ascend -- and pseudo line j - num_slns behind that.  A key-line whose sub-lines straddle
//     the cut contributes the ones in front of it; nothing is written past row M - 1 of an image.
//   - the clip of a row's end point is its record's: the call's own for real lines, the dataset builder's for pseudo lines.
//   - klines / length_klines / angles [B, M]: real key-lines, pseudo key-lines behind them, zeros behind those.
//   - mat_klines2sublines [B, M, M], one row per block: eye(M) with the block [:num_klns, :min(num_slns, M)] replaced by the image's own
//     matrix.  (The reference writes the eye first: a pseudo sub-line has its 1 on the diagonal, and rows num_klns .. num_slns - 1 keep
//     a diagonal 1 inside the real columns.)
// Plain stores; no atomics.  16-byte stores only to desc rows (1 KiB each, 16-byte aligned with the tensor).
#pragma once
#include "lt_token.h"

namespace lt {

struct FsImage { int k0, nk, n0, ns, p0, np; };   // first key-line / count, first sub-line / count, first pseudo line / count
constexpr int FS_TABLE_CHUNK = 32;
struct FsChunk { FsImage img[FS_TABLE_CHUNK]; };

// the per-image table travels in the arguments of one small launch per 32 images (no host buffer has to outlive the call)
static __global__ void fs_table_kernel(const FsChunk c, int first, int count, FsImage* __restrict__ table) {
  const int i = threadIdx.x;
  if (i < count) table[first + i] = c.img[i];
}

// grid B * M, one 64-thread block per output row
static __global__ __launch_bounds__(64) void fs_rows_kernel(
    const LinetrLineRec* __restrict__ recs, const LinetrLineRec* __restrict__ precs, const FsImage* __restrict__ table, int M, double td,
    int T, int height, int width, double clip_x, double clip_y, double pclip_x, double pclip_y, const float* __restrict__ dense_score,
    float* __restrict__ klines, float* __restrict__ length, float* __restrict__ angles, float* __restrict__ sublines,
    float* __restrict__ pnt, float* __restrict__ mask, float* __restrict__ resp, float* __restrict__ angle_sub, float* __restrict__ score,
    float* __restrict__ mat, int* __restrict__ num_klns, int* __restrict__ num_slns) {
  const int b = blockIdx.x / M, j = blockIdx.x - b * M;
  const int64_t n = blockIdx.x;              // (B M T / 4 fits an int, linetr_fixed_size: so does the row)
  const FsImage im = table[b];
  const int ns_c = im.ns < M ? im.ns : M;     // real sub-lines that survive the cut
  if (j == 0 && threadIdx.x == 0) {
    num_klns[b] = im.nk;
    num_slns[b] = im.ns;
  }
  // ---- the sub-line row
  if (j < ns_c) {
    int lo = 0, hi = im.nk - 1;               // last key-line whose first sub-line is not behind j
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (recs[im.k0 + mid].first_sub - im.n0 <= j) lo = mid;
      else hi = mid - 1;
    }
    const LinetrLineRec r = recs[im.k0 + lo];
    const int js = j - (r.first_sub - im.n0);
    if (r.image == b && js >= 0 && js < r.n_sub)      // (records that disagree with the prefix sums: the row is left alone)
      tokenize_subline(r, js, (int)n, td, T, height, width, clip_x, clip_y, dense_score, sublines, pnt, mask, resp, angle_sub, score, nullptr,
                       nullptr);
  } else if (j - im.ns < im.np) {
    const LinetrLineRec r = precs[im.p0 + j - im.ns];
    if (r.image == b)
      tokenize_subline(r, 0, (int)n, td, T, height, width, pclip_x, pclip_y, dense_score, sublines, pnt, mask, resp, angle_sub, score, nullptr,
                       nullptr);
  }
  // ---- the key-line row
  if (threadIdx.x == 32) {
    if (j < im.nk) kline_row(recs[im.k0 + j], clip_x, clip_y, klines + n * 4, length + n, angles + n * 2);
    else if (j - im.nk < im.np) kline_row(precs[im.p0 + j - im.nk], pclip_x, pclip_y, klines + n * 4, length + n, angles + n * 2);
    else {
      klines[n * 4 + 0] = klines[n * 4 + 1] = klines[n * 4 + 2] = klines[n * 4 + 3] = 0.f;
      length[n] = 0.f;
      angles[n * 2 + 0] = angles[n * 2 + 1] = 0.f;
    }
  }
  // ---- row j of the image's [M, M] matrix
  float* row = mat + n * M;
  if (j < im.nk) {
    const LinetrLineRec r = recs[im.k0 + j];
    const float w = k2s_weight(r);
    const int c0 = r.first_sub - im.n0;
    for (int c = threadIdx.x; c < M; c += 64) row[c] = c < ns_c ? ((c >= c0 && c < c0 + r.n_sub) ? w : 0.f) : (c == j ? 1.f : 0.f);
  } else {
    for (int c = threadIdx.x; c < M; c += 64) row[c] = c == j ? 1.f : 0.f;
  }
}

// desc_sublines: one wave per token of the [B * M, T] rows, sampled at the point fs_rows_kernel wrote; grid ceil(B M T / 4), block 256
static __global__ __launch_bounds__(256) void fs_sample_kernel(const float* __restrict__ pnt, int64_t n_tokens, int64_t tokens_per_image,
                                                               const float* __restrict__ nhwc, int Hc, int Wc, int align_corners,
                                                               float* __restrict__ desc) {
  const int64_t tok = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (tok >= n_tokens) return;
  const int lane = threadIdx.x & 63;
  const int64_t img = tok / tokens_per_image;
  const f32x4 o = sample_one(pnt[tok * 2 + 0], pnt[tok * 2 + 1], nhwc + img * Hc * Wc * D, Hc, Wc, align_corners, lane);
  *reinterpret_cast<f32x4*>(desc + tok * D + lane * 4) = o;
}

}  // namespace lt
