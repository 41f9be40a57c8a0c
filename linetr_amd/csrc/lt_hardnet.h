// The HardNet criterion (descriptor_loss.compute_distances_hardnet, evaluations/criteria.py:126-171 of the reference, under its forward
// :173-192 and torch autograd): the hardest positive of every anchor against the hardest negative of the anchor's line and of its
// positive's line; loss scalars and, when asked, the gradient with respect to line_desc0 / line_desc1, from ONE selection.
//   D[a][c] = 2 - 2 <d0[a], d1[c]> (float32, not clipped);  match = assign > 0.3, unmatch = assign <= 0 on the [n][n] part
//   cand = unmatch ? D : 10000;  rowmin[a] = min_c cand[a][c], colmin[c] = min_a cand[a][c]
//   2n anchor lines per item: the n rows of D, then its n columns.  For a line r:
//     pos_r = max(0, largest matched D on the line), an anchor iff pos_r > 0;  p_r = the FIRST index attaining it (torch.max(dim))
//     neg_r = min(own, cross): a row anchor a has own = rowmin[a], cross = colmin[p]; a column anchor c has own = colmin[c],
//             cross = rowmin[p].  No anchor is dropped: lines without an unmatched entry give neg = 10000
//   loss = mean over the V anchors of relu(pos - neg + 1); hardest_positive = max pos; hardest_negative = min neg (may be 10000);
//   V == 0: all three NaN
//   gradient, w = upstream / V: an anchor is live iff pos - neg + 1 > 0 (strict).  It gives +w to its positive entry at p_r alone
//   (nothing is split over tied positives) and -w to the own line if own < cross, to the cross line if own > cross, w / 2 to each if
//   equal (torch.min's backward); on a line the share is divided evenly over every unmatched entry equal to the minimum (amin's
//   backward); entries valued 10000 carry nothing.  An entry of D collects what row anchors and column anchors give it.
//   grad0[a] = -2 sum_c G[a][c] d1[c]        grad1[c] = -2 sum_a G[a][c] d0[a]
// Five launches for a batch of B items with n sub-lines on both sides:
//   val_dot_kernel     (lt_valstep.h) the dot products, once, by exact-fp32 MFMA;
//   hn_select_kernel   grid (row blocks + column blocks, B), the block shapes of lg_select_kernel: per line pos, the first index of the
//                      positive (-1: no anchor), the line's cand minimum and the number of unmatched entries tied at it, in one pass;
//   hn_resolve_kernel  a thread per line: neg, the own / cross split and the live flag of the line's anchor, and the cross weight the
//                      line RECEIVES: a gather over the n anchors of the other direction in ascending order (shares are 0, 1/2, 1);
//   hn_loss_kernel     one block: the scalars in vs_loss_block's order over the lines with pos > 0, V, and the number of live anchors;
//   hn_grad_kernel     grid (tiles, 2, B), lg_grad_kernel's tiling: G is gathered a 64 x 64 tile at a time in LDS from the dots, the
//                      assignment and the two line records of an entry, never stored; a wave walks the non-zeros of its rows in
//                      ascending order.  Not launched for a value-only call.
// Deterministic: no floating-point atomics, every reduction has a fixed order.  Every row of both gradients is written, zeros are +0.
#pragma once
#include "lt_lossgrad.h"

namespace lt {

// (maximum, first index) and (minimum, ties) of a line, combined from two parts in line order: `b` lies behind `a`
__device__ __forceinline__ void hn_join_max(float& pos, int& arg, float opos, int oarg) {
  if (opos > pos || (opos == pos && oarg < arg)) { pos = opos; arg = oarg; }
}
__device__ __forceinline__ void hn_join_min(float& best, int& cnt, float obest, int ocnt) {
  if (obest < best) { best = obest; cnt = ocnt; }
  else if (obest == best) cnt += ocnt;
}
// one entry of a line: d its distance, g its assignment, i its index along the line (ascending per caller: strict > keeps the first)
__device__ __forceinline__ void hn_visit(float d, float g, int i, float& pos, int& arg, float& best, int& cnt) {
  if (g > VS_MATCH && d > pos) { pos = d; arg = i; }
  const bool un = g <= 0.f;
  hn_join_min(best, cnt, un ? d : VS_MASKED, un ? 1 : 0);
}
__device__ __forceinline__ void hn_store_line(float pos, int arg, float best, int cnt, int i, float* __restrict__ lpos, int* __restrict__ larg,
                                              float* __restrict__ lmin, int* __restrict__ lcnt) {
  lpos[i] = pos;
  larg[i] = pos > 0.f ? arg : -1;
  lmin[i] = best;
  lcnt[i] = cnt;
}

// grid (cdiv(n, VS_ROWS) + cdiv(n, VS_COLS), B); the block shapes of lg_select_kernel.  line_pos / line_arg / line_min / line_cnt [B][2n].
__global__ __launch_bounds__(256) void hn_select_kernel(const float* __restrict__ dots, const float* __restrict__ assign, int n,
                                                        float* __restrict__ line_pos, int* __restrict__ line_arg,
                                                        float* __restrict__ line_min, int* __restrict__ line_cnt) {
  __shared__ float s_pos[4][VS_COLS], s_min[4][VS_COLS];
  __shared__ int s_arg[4][VS_COLS], s_cnt[4][VS_COLS];
  const int item = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int row_blocks = (n + VS_ROWS - 1) / VS_ROWS;
  const float* S = dots + (int64_t)item * n * n;
  const float* G = assign + (int64_t)item * (n + 1) * (n + 1);
  float* lpos = line_pos + (int64_t)item * 2 * n;
  int* larg = line_arg + (int64_t)item * 2 * n;
  float* lmin = line_min + (int64_t)item * 2 * n;
  int* lcnt = line_cnt + (int64_t)item * 2 * n;
  float pos = 0.f, best = VS_MASKED;
  int arg = 0x7fffffff, cnt = 0;
  if ((int)blockIdx.x < row_blocks) {
    const int a = blockIdx.x * VS_ROWS + wave;
    if (a >= n) return;
    const float* Sr = S + (int64_t)a * n;
    const float* Gr = G + (int64_t)a * (n + 1);
    for (int c = lane; c < n; c += 64) hn_visit(vs_dist(Sr[c]), Gr[c], c, pos, arg, best, cnt);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {                   // (maximum with the smallest index, minimum with an integer count: order-free)
      hn_join_max(pos, arg, __shfl_xor(pos, o, 64), __shfl_xor(arg, o, 64));
      hn_join_min(best, cnt, __shfl_xor(best, o, 64), __shfl_xor(cnt, o, 64));
    }
    if (lane == 0) hn_store_line(pos, arg, best, cnt, a, lpos, larg, lmin, lcnt);
    return;
  }
  // a column per lane; wave w walks rows w q .. (w + 1) q - 1 in ascending order and the four partial results are combined in wave order
  const int j = ((int)blockIdx.x - row_blocks) * VS_COLS + lane;
  const int jc = min(j, n - 1);
  const int q = (n + 3) / 4, a_lo = wave * q, a_hi = min(n, a_lo + q);
#pragma unroll 4
  for (int a = a_lo; a < a_hi; ++a) hn_visit(vs_dist(S[(int64_t)a * n + jc]), G[(int64_t)a * (n + 1) + jc], a, pos, arg, best, cnt);
  s_pos[wave][lane] = pos; s_arg[wave][lane] = arg; s_min[wave][lane] = best; s_cnt[wave][lane] = cnt;
  __syncthreads();
  if (wave == 0 && j < n) {
#pragma unroll
    for (int w = 1; w < 4; ++w) {
      hn_join_max(pos, arg, s_pos[w][lane], s_arg[w][lane]);
      hn_join_min(best, cnt, s_min[w][lane], s_cnt[w][lane]);
    }
    hn_store_line(pos, arg, best, cnt, n + j, lpos, larg, lmin, lcnt);
  }
}

// what the anchor of a line gives its own line (1, 1/2 or 0; the cross line gets the rest) when it is live, else 0 to both;
// neg = min(own, cross)
__device__ __forceinline__ bool hn_live(float pos, float own, float cross) { return (pos - fminf(own, cross)) + 1.f > 0.f; }
__device__ __forceinline__ float hn_own_share(float own, float cross) { return own < cross ? 1.f : own > cross ? 0.f : 0.5f; }

// grid (cdiv(2n, 256), B): a thread per line.  row_neg [B][2n]: neg of the line's anchor, VS_NONE where it is none; live_arg: the
// positive's index of a LIVE anchor, else -1; neg_share: what every unmatched entry at the line's minimum gets, in units of w.
__global__ __launch_bounds__(256) void hn_resolve_kernel(const float* __restrict__ line_pos, const int* __restrict__ line_arg,
                                                         const float* __restrict__ line_min, const int* __restrict__ line_cnt, int n,
                                                         float* __restrict__ row_neg, int* __restrict__ live_arg,
                                                         float* __restrict__ neg_share) {
  const int item = blockIdx.y, l = blockIdx.x * 256 + threadIdx.x;
  if (l >= 2 * n) return;
  const int64_t base = (int64_t)item * 2 * n;
  const float* lpos = line_pos + base;
  const int* larg = line_arg + base;
  const float* lmin = line_min + base;
  const int mine = l < n ? 0 : n, other = n - mine, i = l - mine;     // the lines of this direction start at `mine`
  const float own = lmin[l];
  const int p = larg[l];
  float weight = 0.f, neg = VS_NONE;
  bool live = false;
  if (p >= 0) {
    const float cross = lmin[other + p];
    neg = fminf(own, cross);
    live = hn_live(lpos[l], own, cross);
    if (live) weight = hn_own_share(own, cross);
  }
  for (int r = 0; r < n; ++r)                             // the anchors of the other direction whose positive lies on this line
    if (larg[other + r] == i) {
      const float theirs = lmin[other + r];
      if (hn_live(lpos[other + r], theirs, own)) weight += 1.f - hn_own_share(theirs, own);
    }
  const int cnt = line_cnt[base + l];
  row_neg[base + l] = neg;
  live_arg[base + l] = live ? p : -1;
  neg_share[base + l] = cnt > 0 ? weight / (float)cnt : 0.f;
}

// One block: vs_loss_block's reduction (the same strides and tree) over the lines that are anchors -- line_arg >= 0, since a HardNet
// negative may be 10000 or, for coincident descriptors, not positive -- and the number of live anchors beside V.
// scalars [3] = loss, hardest_positive, hardest_negative (NaN when V == 0); count [2] = V, live.
__global__ __launch_bounds__(256) void hn_loss_kernel(const float* __restrict__ line_pos, const float* __restrict__ row_neg,
                                                      const int* __restrict__ line_arg, int B, int n, double* __restrict__ scalars,
                                                      long long* __restrict__ count) {
  const int tid = threadIdx.x;
  const int64_t rows = (int64_t)B * 2 * n;
  __shared__ double s_sum[256];
  __shared__ float s_hp[256], s_hn[256];
  __shared__ long long s_v[256], s_live[256];
  double sum = 0.0;
  float hp = -INFINITY, hn = INFINITY;
  long long v = 0, alive = 0;
  for (int64_t i = tid; i < rows; i += 256)
    if (line_arg[i] >= 0) {
      const float pos = line_pos[i], neg = row_neg[i];
      const float t = (pos - neg) + 1.f;
      sum += (double)fmaxf(t, 0.f);
      hp = fmaxf(hp, pos); hn = fminf(hn, neg);
      ++v;
      alive += t > 0.f;
    }
  s_sum[tid] = sum; s_hp[tid] = hp; s_hn[tid] = hn; s_v[tid] = v; s_live[tid] = alive;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {                              // a tree of fixed shape
    if (tid < s) {
      s_sum[tid] += s_sum[tid + s];
      s_hp[tid] = fmaxf(s_hp[tid], s_hp[tid + s]);
      s_hn[tid] = fminf(s_hn[tid], s_hn[tid + s]);
      s_v[tid] += s_v[tid + s];
      s_live[tid] += s_live[tid + s];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const long long V = s_v[0];
    const double nan = __builtin_nan("");
    scalars[0] = V ? s_sum[0] / (double)V : nan;
    scalars[1] = V ? (double)s_hp[0] : nan;
    scalars[2] = V ? (double)s_hn[0] : nan;
    count[0] = V;
    count[1] = s_live[0];
  }
}

// what one line gives an entry, in units of w: `at_pos` the entry is the positive of the line's live anchor; d / unmatch of the entry
__device__ __forceinline__ float hn_share(bool at_pos, float d, bool unmatch, float line_min, float share, float w) {
  return (at_pos ? w : 0.f) - (unmatch && d == line_min ? w * share : 0.f);
}

// grid (cdiv(n, 64), 2, B); lg_grad_kernel's tiling and contraction.  y = 0: rows o0 .. o0 + 63 of grad0, contracted over the rows of
// desc1; y = 1: of grad1, over desc0.  A NULL output: its blocks leave at once.  count: V of hn_loss_kernel; upstream: one float on
// the device, or NULL for 1.
__global__ __launch_bounds__(256) void hn_grad_kernel(const float* __restrict__ desc0, const float* __restrict__ desc1,
                                                      const float* __restrict__ dots, const float* __restrict__ assign, int n,
                                                      const int* __restrict__ live_arg, const float* __restrict__ line_min,
                                                      const float* __restrict__ neg_share, const long long* __restrict__ count,
                                                      const float* __restrict__ upstream, float* __restrict__ grad0,
                                                      float* __restrict__ grad1) {
  __shared__ float Gs[64 * LG_LS];
  __shared__ int s_arg[2][64];                           // [0]: the lines of the tile's rows of D, [1]: of its columns
  __shared__ float s_min[2][64], s_share[2][64];
  const int item = blockIdx.z, side = blockIdx.y, o0 = blockIdx.x * 64;
  float* out = side ? grad1 : grad0;
  if (!out) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* X = (side ? desc0 : desc1) + (int64_t)item * n * D;
  const float* S = dots + (int64_t)item * n * n;
  const float* A = assign + (int64_t)item * (n + 1) * (n + 1);
  const int* larg = live_arg + (int64_t)item * 2 * n;
  const float* lmin = line_min + (int64_t)item * 2 * n;
  const float* lshare = neg_share + (int64_t)item * 2 * n;
  const long long V = *count;
  const float w = V ? (upstream ? *upstream : 1.f) / (float)V : 0.f;
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
      s_arg[which][lane] = in ? larg[r] : -1;
      s_min[which][lane] = lmin[r];
      s_share[which][lane] = in ? lshare[r] : 0.f;
    }
    __syncthreads();
#pragma unroll 4
    for (int i = 0; i < 16; ++i) {
      const int r = wave + 4 * i, a = a0 + r, c = c0 + lane;         // a row of D per wave: coalesced dots and assign
      float g = 0.f;
      if (a < n && c < n) {
        const float d = vs_dist(S[(int64_t)a * n + c]);
        const bool un = A[(int64_t)a * (n + 1) + c] <= 0.f;
        g = hn_share(c == s_arg[0][r], d, un, s_min[0][r], s_share[0][r], w) +
            hn_share(a == s_arg[1][lane], d, un, s_min[1][lane], s_share[1][lane], w);
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
