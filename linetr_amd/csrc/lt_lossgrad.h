// The gradient of the triplet criterion (descriptor_loss, evaluations/criteria.py:59-124,173-192 of the reference, taken through torch
// autograd) with respect to line_desc0 / line_desc1, together with the loss scalars linetr_val_step reports, from ONE selection.
//   loss = mean over the V surviving anchors of relu(pos - neg + 1);  w = upstream / V
//   dL/dD = G: an anchor row gives +w / ties to every entry tied at its positive (amax's backward splits evenly) and -w to its negative
//           (the FIRST index of the smallest semi-hard entry: argmin, then indexing); an entry (a, c) collects what the row anchor a and
//           the column anchor c give it, in that order
//   grad0[a] = -2 sum_c G[a][c] d1[c]        grad1[c] = -2 sum_a G[a][c] d0[a]        (D = 2 - 2 <d0[a], d1[c]>)
// Four launches for a batch of B items with n sub-lines on both sides:
//   val_dot_kernel    (lt_valstep.h) the dot products, once, by exact-fp32 MFMA;
//   lg_select_kernel  grid (row blocks + column blocks, B): val_select_kernel's anchor rows, and per anchor the number of entries tied at
//                     the positive and the index of the negative (0 / -1 where the anchor gives no gradient);
//   lg_loss_kernel    one block: the loss scalars and V by vs_loss_block, the reduction linetr_val_step runs (bit-identical);
//   lg_grad_kernel    grid (tiles, 2, B): 64 rows of grad0 (y = 0) or grad1 (y = 1).  G is formed by GATHER, a 64 x 64 tile at a time in
//                     LDS, from the dots, the assignment and the two anchor records of an entry -- it never reaches memory and nothing
//                     is scattered.  G has a few non-zeros per row (V anchors give at most V (1 + ties) of them), so a wave walks the
//                     non-zeros of its rows in ascending order and adds g x descriptor row to 256 channels in registers: a fixed order.
// Deterministic: no floating-point atomics, every reduction has a fixed order.  Every row of both gradients is written, zeros included.
#pragma once
#include "lt_valstep.h"

namespace lt {

// what lane 0 / a column's lane stores of one anchor row: ties = 0 and negative = -1 unless the anchor survives with an active relu
// (pos - neg + 1 > 0, strict like torch's threshold_backward; the semi-hard window makes it 0.5 .. 1)
__device__ __forceinline__ void lg_store_anchor(float pos, float neg, int arg, int ties, int i, float* __restrict__ rpos,
                                                float* __restrict__ rneg, int* __restrict__ rties, int* __restrict__ rarg) {
  const bool kept = neg < INFINITY;
  const bool live = kept && (pos - neg) + 1.f > 0.f;
  rpos[i] = pos;
  rneg[i] = kept ? neg : VS_NONE;
  rties[i] = live ? ties : 0;
  rarg[i] = live ? arg : -1;
}

// grid (cdiv(n, VS_ROWS) + cdiv(n, VS_COLS), B); the block shapes of val_select_kernel.  row_pos / row_neg / row_ties / row_arg [B][2n].
__global__ __launch_bounds__(256) void lg_select_kernel(const float* __restrict__ dots, const float* __restrict__ assign, int n,
                                                        float* __restrict__ row_pos, float* __restrict__ row_neg,
                                                        int* __restrict__ row_ties, int* __restrict__ row_arg) {
  __shared__ float s_val[4][VS_COLS];
  __shared__ int s_arg[4][VS_COLS];
  __shared__ int s_ties[4][VS_COLS];
  const int item = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int row_blocks = (n + VS_ROWS - 1) / VS_ROWS;
  const float* S = dots + (int64_t)item * n * n;
  const float* G = assign + (int64_t)item * (n + 1) * (n + 1);
  float* rpos = row_pos + (int64_t)item * 2 * n;
  float* rneg = row_neg + (int64_t)item * 2 * n;
  int* rties = row_ties + (int64_t)item * 2 * n;
  int* rarg = row_arg + (int64_t)item * 2 * n;
  if ((int)blockIdx.x < row_blocks) {
    const int a = blockIdx.x * VS_ROWS + wave;
    if (a >= n) return;
    const float* Sr = S + (int64_t)a * n;
    const float* Gr = G + (int64_t)a * (n + 1);
    float pos = 0.f;
    for (int c = lane; c < n; c += 64)
      if (Gr[c] > VS_MATCH) pos = fmaxf(pos, vs_dist(Sr[c]));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) pos = fmaxf(pos, __shfl_xor(pos, o, 64));
    float neg = INFINITY;
    int arg = 0x7fffffff, ties = 0;
    if (pos > 0.f) {                                     // (wave-uniform) an anchor
      const float pm = pos + VS_MARGIN;
      for (int c = lane; c < n; c += 64) {
        const float d = vs_dist(Sr[c]), g = Gr[c];
        ties += g > VS_MATCH && d == pos;
        const float v = vs_neg_value(d, g);
        if (vs_semi_hard(v, pos, pm) && v < neg) { neg = v; arg = c; }     // ascending c per lane: strict < keeps the first
      }
      vs_wave_argmin(neg, arg);
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) ties += __shfl_xor(ties, o, 64);    // (an integer sum: order-independent)
    }
    if (lane == 0) lg_store_anchor(pos, neg, arg, ties, a, rpos, rneg, rties, rarg);
    return;
  }
  // a column per lane; wave w walks rows w q .. (w + 1) q - 1 in ascending order and the four partial results are combined in wave
  // order, so a tie keeps the first row
  const int j = ((int)blockIdx.x - row_blocks) * VS_COLS + lane;
  const int jc = min(j, n - 1);
  const int q = (n + 3) / 4, a_lo = wave * q, a_hi = min(n, a_lo + q);
  float pos = 0.f;
#pragma unroll 4
  for (int a = a_lo; a < a_hi; ++a)
    if (G[(int64_t)a * (n + 1) + jc] > VS_MATCH) pos = fmaxf(pos, vs_dist(S[(int64_t)a * n + jc]));
  s_val[wave][lane] = pos;
  __syncthreads();
  pos = fmaxf(fmaxf(s_val[0][lane], s_val[1][lane]), fmaxf(s_val[2][lane], s_val[3][lane]));
  __syncthreads();
  float neg = INFINITY;
  int arg = 0x7fffffff, ties = 0;
  if (pos > 0.f) {
    const float pm = pos + VS_MARGIN;
#pragma unroll 4
    for (int a = a_lo; a < a_hi; ++a) {
      const float d = vs_dist(S[(int64_t)a * n + jc]), g = G[(int64_t)a * (n + 1) + jc];
      ties += g > VS_MATCH && d == pos;
      const float v = vs_neg_value(d, g);
      if (vs_semi_hard(v, pos, pm) && v < neg) { neg = v; arg = a; }
    }
  }
  s_val[wave][lane] = neg; s_arg[wave][lane] = arg; s_ties[wave][lane] = ties;
  __syncthreads();
  if (wave == 0 && j < n) {
    neg = s_val[0][lane]; arg = s_arg[0][lane]; ties = s_ties[0][lane];
#pragma unroll
    for (int w = 1; w < 4; ++w) {
      if (s_val[w][lane] < neg) { neg = s_val[w][lane]; arg = s_arg[w][lane]; }
      ties += s_ties[w][lane];
    }
    lg_store_anchor(pos, neg, arg, ties, n + j, rpos, rneg, rties, rarg);
  }
}

// one block: loss, hardest_positive, hardest_negative and V, as val_final_kernel's last block computes them
__global__ __launch_bounds__(256) void lg_loss_kernel(const float* __restrict__ row_pos, const float* __restrict__ row_neg, int B, int n,
                                                      double* __restrict__ scalars, long long* __restrict__ count) {
  vs_loss_block(row_pos, row_neg, (int64_t)B * 2 * n, scalars, count);
}

// what one anchor gives an entry of its row: `d`, `match` of the entry, `other` its index along the row; pos / ties / neg the anchor's record
__device__ __forceinline__ float lg_share(float d, bool match, int other, float pos, int ties, int neg, float w) {
  if (ties <= 0) return 0.f;                             // no gradient from this row (a live anchor has at least one tied positive)
  return (match && d == pos ? w / (float)ties : 0.f) - (other == neg ? w : 0.f);
}

constexpr int LG_LS = 65;         // row stride of the G tile in LDS: conflict-free rows and columns

// grid (cdiv(n, 64), 2, B).  y = 0: rows o0 .. o0 + 63 of grad0, contracted over the rows of desc1; y = 1: of grad1, over desc0.
// A NULL output: its blocks leave at once.  count: V of lg_loss_kernel; upstream: one float on the device, or NULL for 1.
__global__ __launch_bounds__(256) void lg_grad_kernel(const float* __restrict__ desc0, const float* __restrict__ desc1,
                                                      const float* __restrict__ dots, const float* __restrict__ assign, int n,
                                                      const float* __restrict__ row_pos, const int* __restrict__ row_ties,
                                                      const int* __restrict__ row_arg, const long long* __restrict__ count,
                                                      const float* __restrict__ upstream, float* __restrict__ grad0,
                                                      float* __restrict__ grad1) {
  __shared__ float Gs[64 * LG_LS];
  __shared__ float s_pos[2][64];                         // [0]: the row anchors of the tile's rows of D, [1]: the column anchors of its columns
  __shared__ int s_ties[2][64], s_neg[2][64];
  const int item = blockIdx.z, side = blockIdx.y, o0 = blockIdx.x * 64;
  float* out = side ? grad1 : grad0;
  if (!out) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* X = (side ? desc0 : desc1) + (int64_t)item * n * D;
  const float* S = dots + (int64_t)item * n * n;
  const float* A = assign + (int64_t)item * (n + 1) * (n + 1);
  const float* rpos = row_pos + (int64_t)item * 2 * n;
  const int* rties = row_ties + (int64_t)item * 2 * n;
  const int* rarg = row_arg + (int64_t)item * 2 * n;
  const long long V = *count;
  const float w = V ? (upstream ? *upstream : 1.f) / (float)V : 0.f;  // (V == 0: no anchor has ties > 0; every share is 0)
  f32x4 acc[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < n; k0 += 64) {
    const int a0 = side ? k0 : o0, c0 = side ? o0 : k0;  // the tile of D: rows a0 .., columns c0 ..
    __syncthreads();                                     // the tile before has been read
    if (tid < 128) {
      const int which = tid >> 6, i = (which ? c0 : a0) + lane;
      const bool in = i < n;
      const int r = which * n + min(i, n - 1);
      s_pos[which][lane] = rpos[r];
      s_ties[which][lane] = in ? rties[r] : 0;
      s_neg[which][lane] = in ? rarg[r] : -1;
    }
    __syncthreads();
#pragma unroll 4
    for (int i = 0; i < 16; ++i) {
      const int r = wave + 4 * i, a = a0 + r, c = c0 + lane;         // a row of D per wave: coalesced dots and assign
      float g = 0.f;
      if (a < n && c < n) {
        const float d = vs_dist(S[(int64_t)a * n + c]);
        const bool match = A[(int64_t)a * (n + 1) + c] > VS_MATCH;
        g = lg_share(d, match, c, s_pos[0][r], s_ties[0][r], s_neg[0][r], w) +
            lg_share(d, match, a, s_pos[1][lane], s_ties[1][lane], s_neg[1][lane], w);
      }
      Gs[side ? lane * LG_LS + r : r * LG_LS + lane] = g;            // [output row][contracted row]
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const float g = Gs[(wave * 16 + j) * LG_LS + lane];
      unsigned long long m = __ballot(g != 0.f);
      while (m) {                                        // (wave-uniform) the non-zeros of the row, ascending
        const int k = __ffsll(m) - 1;
        m &= m - 1;
        const float gk = -2.f * __shfl(g, k, 64);
        const f32x4 v = *reinterpret_cast<const f32x4*>(X + (int64_t)(k0 + k) * D + lane * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[j][e] = fmaf(gk, v[e], acc[j][e]);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int o = o0 + wave * 16 + j;
    if (o < n) *reinterpret_cast<f32x4*>(out + ((int64_t)item * n + o) * D + lane * 4) = acc[j];      // (a row without a non-zero: +0)
  }
}

}  // namespace lt
