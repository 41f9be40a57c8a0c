// The validation step that follows the batched forward (train.py:198-240 of the reference) on the device, forward only:
//   descriptor_loss      evaluations/criteria.py:59-124,173-192   semi-hard triplet selection + relu(pos - neg + 1) mean
//   nn_matcher_batches   evaluations/matcher.py:51-102            nearest neighbour on squared distances, threshold, mutual check
//   Evaluate_PR          evaluations/evaluate_pr.py:10-35         TP / FP / FN / TN, precision / recall / F1 per item
// and the ground-truth matrix train.py:176-183 scatters from the loader's match list.
// Three launches for a batch of B items with n sub-lines on both sides:
//   val_dot_kernel     grid (tiles, tiles, B): <d0[a], d1[c]> ONCE, by the matcher's exact-fp32 MFMA tile (dot_tile_64x64, lt_parts.h:
//                      a selection must not inherit a split's error), and the squared norms of both sides;
//   val_select_kernel  grid (row blocks + column blocks, B): per anchor row (n rows of D, then n rows of D^T) the hardest positive
//                      and its semi-hard negative; per row / column the first-index argmin of the matcher's score;
//   val_final_kernel   grid (B + 1): per item threshold + mutual check + the four counts and three scores; one block for the loss.
// Both formulas read the one set of dot products:   D = 2 - 2 dot   (criterion, no clip)   score = max((|d0|^2 + |d1|^2) - 2 dot, 0).
// Deterministic: every reduction has a fixed order (max / min / integer sums are order-independent, the loss sum is a float64 tree
// of fixed shape); no floating-point atomics.
#pragma once
#include "lt_parts.h"

namespace lt {

constexpr float VS_MATCH = 0.3f;       // assign > VS_MATCH: a match (criteria.py:65); assign <= 0: an unmatch (:66)
constexpr float VS_MARGIN = 0.5f;      // semi-hard window above the positive (criteria.py:100-102)
constexpr float VS_MASKED = 10000.f;   // what an entry that is not an unmatch counts as among the negatives (criteria.py:94-95)
constexpr float VS_NONE = -1.f;        // row_neg of a row that is no anchor, or an anchor without a semi-hard negative (a real one is > 0)
constexpr int VS_ROWS = 4;             // anchor rows of D per row block (one wave each)
constexpr int VS_COLS = 64;            // anchor rows of D^T per column block (one lane each, the rows of D split over the 4 waves)

// the criterion's distance and the matcher's score of one dot product
__device__ __forceinline__ float vs_dist(float dot) { return 2.f - 2.f * dot; }
__device__ __forceinline__ float vs_score(float sq_a, float sq_c, float dot) { return fmaxf((sq_a + sq_c) - 2.f * dot, 0.f); }
// the value an entry has among the negatives of an anchor, and whether it is semi-hard for that anchor (both compares strict)
__device__ __forceinline__ float vs_neg_value(float d, float assign) { return assign <= 0.f ? d : VS_MASKED; }
__device__ __forceinline__ bool vs_semi_hard(float v, float pos, float pos_margin) { return v > pos && v < pos_margin; }

// |row|^2 of the 64 rows r0 .. r0 + 63 of X [n][256] by the 256 threads of a block: four threads per row, 64 consecutive channels
// each in channel order, the four partial sums added in quarter order.
__device__ __forceinline__ void vs_row_norms(const float* __restrict__ X, int n, int r0, float* __restrict__ sq) {
  const int tid = threadIdx.x, row = r0 + (tid >> 2), q = tid & 3;
  const f32x4* p = reinterpret_cast<const f32x4*>(X + (int64_t)min(row, n - 1) * D + q * 64);
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const f32x4 v = p[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) s = fmaf(v[e], v[e], s);
  }
  const int base = (tid & 63) & ~3;
  const float s0 = __shfl(s, base, 64), s1 = __shfl(s, base + 1, 64), s2 = __shfl(s, base + 2, 64), s3 = __shfl(s, base + 3, 64);
  if (q == 0 && row < n) sq[row] = ((s0 + s1) + s2) + s3;
}

// dots [B][n][n], sq0 / sq1 [B][n]; grid (cdiv(n,64), cdiv(n,64), B)
__global__ __launch_bounds__(256) void val_dot_kernel(const float* __restrict__ desc0, const float* __restrict__ desc1, int n,
                                                      float* __restrict__ dots, float* __restrict__ sq0, float* __restrict__ sq1) {
  __shared__ __attribute__((aligned(16))) float As[64 * DOT_LS];
  __shared__ __attribute__((aligned(16))) float Bs[64 * DOT_LS];
  const int item = blockIdx.z, a0 = blockIdx.y * 64, b0 = blockIdx.x * 64;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wa = wave >> 1, wb = wave & 1;
  const float* A = desc0 + (int64_t)item * n * D;
  const float* B = desc1 + (int64_t)item * n * D;
  const f32x16 acc = dot_tile_64x64(A, n, a0, B, n, b0, As, Bs);
  float* S = dots + (int64_t)item * n * n;
  const int col = b0 + wb * 32 + (lane & 31);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = a0 + wa * 32 + dot_tile_row(r, lane);
    if (row < n && col < n) S[(int64_t)row * n + col] = acc[r];
  }
  // the first tile column owns the norms of its rows of image 0, the first tile row those of its rows of image 1
  if (blockIdx.x == 0) vs_row_norms(A, n, a0, sq0 + (int64_t)item * n);
  if (blockIdx.y == 0) vs_row_norms(B, n, b0, sq1 + (int64_t)item * n);
}

// first-index minimum of (value, index) pairs across a wave
__device__ __forceinline__ void vs_wave_argmin(float& best, int& arg) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int oa = __shfl_xor(arg, o, 64);
    if (ov < best || (ov == best && oa < arg)) { best = ov; arg = oa; }
  }
}

// grid (cdiv(n, VS_ROWS) + cdiv(n, VS_COLS), B).  assign: [B][n+1][n+1] (the dustbin row and column are not read).
//   row blocks:    anchor row a of D (row_pos / row_neg [item][a]), row argmin + minimum of the score, "row a has a ground truth";
//   column blocks: anchor row n + j = row j of D^T (row_pos / row_neg [item][n + j]), column argmin of the score.
__global__ __launch_bounds__(256) void val_select_kernel(const float* __restrict__ dots, const float* __restrict__ sq0,
                                                         const float* __restrict__ sq1, const float* __restrict__ assign, int n,
                                                         float* __restrict__ row_pos, float* __restrict__ row_neg,
                                                         int* __restrict__ row_arg, float* __restrict__ row_min,
                                                         int* __restrict__ col_arg, int* __restrict__ row_gt) {
  __shared__ float s_val[4][VS_COLS];
  __shared__ float s_best[4][VS_COLS];
  __shared__ int s_arg[4][VS_COLS];
  const int item = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int row_blocks = (n + VS_ROWS - 1) / VS_ROWS;
  const float* S = dots + (int64_t)item * n * n;
  const float* G = assign + (int64_t)item * (n + 1) * (n + 1);
  const float* q0 = sq0 + (int64_t)item * n;
  const float* q1 = sq1 + (int64_t)item * n;
  float* rpos = row_pos + (int64_t)item * 2 * n;
  float* rneg = row_neg + (int64_t)item * 2 * n;
  if ((int)blockIdx.x < row_blocks) {
    const int a = blockIdx.x * VS_ROWS + wave;
    if (a >= n) return;
    const float* Sr = S + (int64_t)a * n;
    const float* Gr = G + (int64_t)a * (n + 1);
    const float sa = q0[a];
    float pos = 0.f, best = INFINITY;                    // pos = max(0, .): never negative (the reference's amax can be, where every
    int arg = 0x7fffffff, gt = 0;                        // column is a match; no anchor either way)
    for (int c = lane; c < n; c += 64) {
      const float dot = Sr[c], g = Gr[c];
      if (g > VS_MATCH) pos = fmaxf(pos, vs_dist(dot));
      gt |= g > 0.f;
      const float sc = vs_score(sa, q1[c], dot);
      if (sc < best) { best = sc; arg = c; }             // ascending c per lane: strict < keeps the first
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) pos = fmaxf(pos, __shfl_xor(pos, o, 64));
    vs_wave_argmin(best, arg);
    gt = __any(gt);
    float neg = INFINITY;
    if (pos > 0.f) {                                     // (wave-uniform) an anchor: its semi-hard negatives
      const float pm = pos + VS_MARGIN;
      for (int c = lane; c < n; c += 64) {
        const float v = vs_neg_value(vs_dist(Sr[c]), Gr[c]);
        if (vs_semi_hard(v, pos, pm)) neg = fminf(neg, v);
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) neg = fminf(neg, __shfl_xor(neg, o, 64));
    }
    if (lane == 0) {
      rpos[a] = pos;
      rneg[a] = neg < INFINITY ? neg : VS_NONE;
      row_arg[(int64_t)item * n + a] = arg == 0x7fffffff ? 0 : arg;     // a row without an ordered score: index 0, minimum inf
      row_min[(int64_t)item * n + a] = best;
      row_gt[(int64_t)item * n + a] = gt ? 1 : 0;
    }
    return;
  }
  // a column per lane (coalesced rows of dots and assign); wave w walks rows w q .. (w + 1) q - 1 in ascending order and the four
  // partial results are combined in wave order, so a tie keeps the first row
  const int j = ((int)blockIdx.x - row_blocks) * VS_COLS + lane;
  const int jc = min(j, n - 1);
  const int q = (n + 3) / 4, a_lo = wave * q, a_hi = min(n, a_lo + q);
  const float sc1 = q1[jc];
  float pos = 0.f, best = INFINITY;
  int arg = 0;
#pragma unroll 4
  for (int a = a_lo; a < a_hi; ++a) {
    const float dot = S[(int64_t)a * n + jc], g = G[(int64_t)a * (n + 1) + jc];
    if (g > VS_MATCH) pos = fmaxf(pos, vs_dist(dot));
    const float sc = vs_score(q0[a], sc1, dot);
    if (sc < best) { best = sc; arg = a; }
  }
  s_val[wave][lane] = pos; s_best[wave][lane] = best; s_arg[wave][lane] = arg;
  __syncthreads();
  pos = s_val[0][lane]; best = s_best[0][lane]; arg = s_arg[0][lane];
#pragma unroll
  for (int w = 1; w < 4; ++w) {
    pos = fmaxf(pos, s_val[w][lane]);
    if (s_best[w][lane] < best) { best = s_best[w][lane]; arg = s_arg[w][lane]; }
  }
  __syncthreads();
  float neg = INFINITY;
  if (pos > 0.f) {
    const float pm = pos + VS_MARGIN;
#pragma unroll 4
    for (int a = a_lo; a < a_hi; ++a) {
      const float v = vs_neg_value(vs_dist(S[(int64_t)a * n + jc]), G[(int64_t)a * (n + 1) + jc]);
      if (vs_semi_hard(v, pos, pm)) neg = fminf(neg, v);
    }
  }
  s_val[wave][lane] = neg;
  __syncthreads();
  if (wave == 0 && j < n) {
    neg = fminf(fminf(s_val[0][lane], s_val[1][lane]), fminf(s_val[2][lane], s_val[3][lane]));
    rpos[n + j] = pos;
    rneg[n + j] = neg < INFINITY ? neg : VS_NONE;
    col_arg[(int64_t)item * n + j] = arg;
  }
}

// The device image of the result block (byte offsets from linetr_val_step_output_bytes):
//   scalars f64 [3] = loss, hardest_positive, hardest_negative | count i64 [1] = V | counts i32 [B][4] = TP, FP, FN, TN |
//   scores f64 [B][3] = precision, recall, f1
struct ValOut { double* scalars; long long* count; int* counts; double* scores; };

// The loss over the V anchors that kept a negative (rows: all B * 2n anchor rows), by one block of 256 threads: a float64 sum of fixed
// shape, hardest positive / negative, V.  scalars [3] = loss, hardest_positive, hardest_negative (NaN when V == 0).
__device__ __forceinline__ void vs_loss_block(const float* __restrict__ row_pos, const float* __restrict__ row_neg, int64_t rows,
                                              double* __restrict__ scalars, long long* __restrict__ count) {
  const int tid = threadIdx.x;
  __shared__ double s_sum[256];
  __shared__ float s_hp[256], s_hn[256];
  __shared__ long long s_v[256];
  double sum = 0.0;
  float hp = -INFINITY, hn = INFINITY;
  long long v = 0;
  for (int64_t i = tid; i < rows; i += 256) {
    const float neg = row_neg[i];
    if (neg > 0.f) {
      const float pos = row_pos[i];
      sum += (double)fmaxf((pos - neg) + 1.f, 0.f);
      hp = fmaxf(hp, pos); hn = fminf(hn, neg);
      ++v;
    }
  }
  s_sum[tid] = sum; s_hp[tid] = hp; s_hn[tid] = hn; s_v[tid] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {                              // a tree of fixed shape
    if (tid < s) {
      s_sum[tid] += s_sum[tid + s];
      s_hp[tid] = fmaxf(s_hp[tid], s_hp[tid + s]);
      s_hn[tid] = fminf(s_hn[tid], s_hn[tid + s]);
      s_v[tid] += s_v[tid + s];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const long long V = s_v[0];
    const double nan = __builtin_nan("");
    scalars[0] = V ? s_sum[0] / (double)V : nan;                   // V == 0: the reference has nothing to stack (criteria.py:117)
    scalars[1] = V ? (double)s_hp[0] : nan;
    scalars[2] = V ? (double)s_hn[0] : nan;
    count[0] = V;
  }
}

// grid (B + 1).  Blocks 0 .. B-1: match01 of an item (threshold strict, optional mutual check), its counts (evaluate_pr.py:10-22:
// ground truth assign > 0; FP = rows without a ground truth that have a prediction) and scores (:28-30, float64, eps 1e-5, x 100).
// Block B: the loss over the V anchors that kept a negative, summed in float64.
__global__ __launch_bounds__(256) void val_final_kernel(const float* __restrict__ row_pos, const float* __restrict__ row_neg,
                                                        const int* __restrict__ row_arg, const float* __restrict__ row_min,
                                                        const int* __restrict__ col_arg, const int* __restrict__ row_gt,
                                                        const float* __restrict__ assign, int B, int n, double thr, int mutual,
                                                        int* __restrict__ match01, ValOut out) {
  const int tid = threadIdx.x;
  if ((int)blockIdx.x < B) {
    __shared__ int s_cnt[3];                                       // TP, rows with a ground truth, TN
    const int item = blockIdx.x;
    if (tid < 3) s_cnt[tid] = 0;
    __syncthreads();
    const float* G = assign + (int64_t)item * (n + 1) * (n + 1);
    int tp = 0, npos = 0, tn = 0;
    for (int a = tid; a < n; a += 256) {
      const int64_t i = (int64_t)item * n + a;
      const int c = row_arg[i];
      bool keep = (double)row_min[i] < thr;                        // (float64 threshold: NumPy compares a float32 score with a Python float)
      if (mutual) keep = keep && col_arg[(int64_t)item * n + c] == a;
      const int m = keep ? c : -1;
      match01[i] = m;
      const int gt = row_gt[i];
      npos += gt;
      tp += m >= 0 && G[(int64_t)a * (n + 1) + m] > 0.f;
      tn += !gt && m < 0;
    }
    atomicAdd(&s_cnt[0], tp); atomicAdd(&s_cnt[1], npos); atomicAdd(&s_cnt[2], tn);   // (integer sums: order-independent)
    __syncthreads();
    if (tid == 0) {
      const int TP = s_cnt[0], FN = s_cnt[1] - TP, TN = s_cnt[2], FP = (n - s_cnt[1]) - TN;
      int* c = out.counts + 4 * item;
      c[0] = TP; c[1] = FP; c[2] = FN; c[3] = TN;
      const double eps = 0.00001;
      const double p = (double)TP / ((double)(TP + FP) + eps) * 100.0;
      const double r = (double)TP / ((double)(TP + FN) + eps) * 100.0;
      double* s = out.scores + 3 * item;
      s[0] = p; s[1] = r; s[2] = (p + r) == 0.0 ? 0.0 : 2.0 * p * r / (p + r);       // (nan_to_num of 0 / 0)
    }
    return;
  }
  vs_loss_block(row_pos, row_neg, (int64_t)B * 2 * n, out.scalars, out.count);
}

// train.py:176-183: assign [B][n+1][n+1] = 0, then 1 at (lmatches[b][m][0], lmatches[b][m][1]) for every row m whose first entry is
// not -1.  The caller zero-fills; equal pairs store the same value.  An index outside 0 .. n is skipped.
__global__ __launch_bounds__(256) void val_assign_kernel(const int* __restrict__ lmatches, int B, int M, int n, float* __restrict__ assign) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)B * M) return;
  const int r = lmatches[2 * i], c = lmatches[2 * i + 1];
  if (r < 0 || r > n || c < 0 || c > n) return;
  assign[(i / M) * (int64_t)(n + 1) * (n + 1) + (int64_t)r * (n + 1) + c] = 1.f;
}

}  // namespace lt
