// SuperPoint's key-point branch on the device (models/superpoint.py:48-63 simple_nms, :66-78 remove_borders / top_k_keypoints,
// :81-93 sample_descriptors, and the per-image loop of :168-187): non-maximum suppression, threshold, border filter, ordered
// compaction, optional top-k and the descriptor lookup for a whole batch, with nothing decided by an atomic's arrival order.
//   sp_nms_kernel          score map -> one bit per pixel (kept && score > threshold && inside the border)
//   sp_kp_scan_kernel      bits -> per-row exclusive offsets inside the image + the image's count
//   sp_kp_offsets_kernel   counts -> packed offsets cu_kp[B+1]
//   sp_kp_emit_kernel      bits -> key points in row-major order (torch.nonzero's), or 64-bit sort keys for the top-k
//   sp_kp_topk_kernel      the k largest scores in descending order, ties to the lower row-major index
// (the descriptor lookup of the branch, sp_kp_desc_kernel, sits next to the sampler it shares: lt_token.h)
// Every step of the detector is a compare, a select or a copy: its key points and scores equal torch's bit for bit.
#pragma once
#include "lt_parts.h"

namespace lt {

constexpr int KP_TW = 64;         // tile width: one wave covers a tile row, its ballot is two mask words
constexpr int KP_MAX_R = 8;       // nms_radius
constexpr int KP_MAX_K = 4096;    // max_keypoints (the top-k sorts in LDS)

// tile height by radius: the halo is 5 r on every side (five pools, each widens the dependence by r) and a pixel of the haloed
// region costs 10 bytes of LDS (scores, the row pass's result, two byte masks).  r <= 4: 72 x 104 pixels, 75 KB, two blocks per
// CU; r = 8: 96 x 144 pixels, 138 KB, one block.
inline int kp_tile_h(int r) { return r <= 4 ? 32 : 16; }
inline size_t kp_nms_lds(int r) { return (size_t)(kp_tile_h(r) + 10 * r) * (KP_TW + 10 * r) * 10; }

// (2r+1)^2 maximum of src over the region that shrinks by r per stage, separable: a row pass into tmp (all rows still valid,
// the columns of the result), then a column pass that hands every result to op(y, x, maximum).  The maximum is a compare and a
// select, not v_max_f32: the operand's bits survive whatever the denormal mode.  Stage k reads what stage k - 1
// left valid, [(k-1) r, size - (k-1) r), and is valid on [k r, size - k r).  Lanes run along x in both passes: no bank conflicts.
template <typename T, typename Src, typename Op>
__device__ __forceinline__ void kp_pool(int k, int r, int RH, int RW, T* __restrict__ tmp, Src src, Op op) {
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int ilo = (k - 1) * r, olo = k * r;
  for (int y = ilo + ty; y < RH - ilo; y += 4)
    for (int x = olo + tx; x < RW - olo; x += 64) {
      T m = src(y * RW + x - r);
      for (int d = 1 - r; d <= r; ++d) { const T v = src(y * RW + x + d); m = v > m ? v : m; }
      tmp[y * RW + x] = m;
    }
  __syncthreads();
  for (int y = olo + ty; y < RH - olo; y += 4)
    for (int x = olo + tx; x < RW - olo; x += 64) {
      T m = tmp[(y - r) * RW + x];
      for (int d = 1 - r; d <= r; ++d) { const T v = tmp[(y + d) * RW + x]; m = v > m ? v : m; }
      op(y, x, m);
    }
  __syncthreads();
}

// simple_nms + threshold + remove_borders for one TH x 64 tile of one image.  grid (ceil(W/64), ceil(H/TH), B), block 256,
// dynamic LDS kp_nms_lds(r).
//   keep = s == pool(s);  twice: near = pool(keep) > 0;  rest = near ? 0 : s;  keep |= (rest == pool(rest)) & ~near
// pool pads with -inf: pixels outside the image hold -inf in S and 0 in both masks.  `rest` is never stored.
// mask [B][H][Wm] gets bit (x & 31) of word x / 32 = keep && s > thr && inside the border; every word is written.
__global__ __launch_bounds__(256) void sp_nms_kernel(const float* __restrict__ score, int H, int W, int r, int TH, float thr,
                                                     int border, unsigned* __restrict__ mask, int Wm) {
  extern __shared__ __attribute__((aligned(16))) unsigned char kp_lds[];
  const int RW = KP_TW + 10 * r, RH = TH + 10 * r, px = RW * RH;
  float* S = reinterpret_cast<float*>(kp_lds);
  float* T = S + px;
  unsigned char* K = reinterpret_cast<unsigned char*>(T + px);
  unsigned char* N = K + px;
  unsigned char* TB = reinterpret_cast<unsigned char*>(T);      // the byte pools' row pass (T is free between float pools)
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int b = blockIdx.z, x0 = blockIdx.x * KP_TW - 5 * r, y0 = blockIdx.y * TH - 5 * r;
  const float* img = score + (int64_t)b * H * W;
  auto in_img = [&](int y, int x) { const int gy = y0 + y, gx = x0 + x; return gy >= 0 && gy < H && gx >= 0 && gx < W; };
  for (int y = ty; y < RH; y += 4)
    for (int x = tx; x < RW; x += 64)
      S[y * RW + x] = in_img(y, x) ? img[(int64_t)(y0 + y) * W + (x0 + x)] : -INFINITY;
  __syncthreads();
  kp_pool<float>(1, r, RH, RW, T, [&](int i) { return S[i]; },
                 [&](int y, int x, float m) { const int i = y * RW + x; K[i] = in_img(y, x) && S[i] == m; });
  for (int round = 0; round < 2; ++round) {
    kp_pool<unsigned char>(2 + 2 * round, r, RH, RW, TB, [&](int i) { return K[i]; },
                           [&](int y, int x, unsigned char m) { N[y * RW + x] = in_img(y, x) && m; });
    kp_pool<float>(3 + 2 * round, r, RH, RW, T, [&](int i) { return N[i] ? 0.f : S[i]; },
                   [&](int y, int x, float m) {
                     const int i = y * RW + x;
                     const float rest = N[i] ? 0.f : S[i];
                     if (in_img(y, x) && !N[i] && rest == m) K[i] = 1;
                     if (round == 1) {      // last stage: exactly the tile.  N becomes the output predicate
                       const int gy = y0 + y, gx = x0 + x;
                       N[i] = in_img(y, x) && K[i] && S[i] > thr && gy >= border && gy < H - border && gx >= border && gx < W - border;
                     }
                   });
  }
  for (int y = 5 * r + ty; y < 5 * r + TH; y += 4) {      // a wave = one tile row
    const int gy = y0 + y;
    if (gy >= H) break;
    const unsigned long long bal = __ballot(N[y * RW + 5 * r + tx] != 0);
    if (tx == 0) {
      unsigned* row = mask + ((int64_t)b * H + gy) * Wm;
      const int wi = blockIdx.x * 2;
      if (wi < Wm) row[wi] = (unsigned)bal;
      if (wi + 1 < Wm) row[wi + 1] = (unsigned)(bal >> 32);
    }
  }
}

// one block per image: row_off[b][y] = number of set bits in rows < y, found[b] = the image's count (uncapped)
__global__ __launch_bounds__(256) void sp_kp_scan_kernel(const unsigned* __restrict__ mask, int H, int Wm, int* __restrict__ row_off,
                                                         int* __restrict__ found) {
  __shared__ int part[256];
  const int b = blockIdx.x, t = threadIdx.x;
  int carry = 0;
  for (int base = 0; base < H; base += 256) {
    const int y = base + t;
    int c = 0;
    if (y < H) {
      const unsigned* row = mask + ((int64_t)b * H + y) * Wm;
      for (int w = 0; w < Wm; ++w) c += __popc(row[w]);
    }
    int sum;
    const int ex = kp_block_scan(c, part, sum);
    if (y < H) row_off[(int64_t)b * H + y] = carry + ex;
    carry += sum;
  }
  if (t == 0) found[b] = carry;
}

// one block: cu_kp[b] = sum over earlier images of what they emit, min(found, cap) and at most k with a top-k
__global__ __launch_bounds__(256) void sp_kp_offsets_kernel(const int* __restrict__ found, int B, int cap, int k, int* __restrict__ cu_kp) {
  __shared__ int part[256];
  const int t = threadIdx.x;
  int carry = 0;
  for (int base = 0; base < B; base += 256) {
    const int i = base + t;
    int c = i < B ? min(found[i], cap) : 0;
    if (k >= 0) c = min(c, k);
    int sum;
    const int ex = kp_block_scan(c, part, sum);
    if (i < B) cu_kp[i] = carry + ex;
    carry += sum;
  }
  if (t == 0) cu_kp[B] = carry;
}

// scores as unsigned integers of the same order, and back
__device__ __forceinline__ unsigned kp_ordered(float f) {
  const unsigned u = __builtin_bit_cast(unsigned, f);
  return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float kp_unordered(unsigned o) {
  return __builtin_bit_cast(float, (o & 0x80000000u) ? (o ^ 0x80000000u) : ~o);
}

// One wave per image row: the rank of a set bit is row_off + popcounts of the words (and bits) in front of it.  Without a top-k the
// key point goes to cu_kp[b] + rank as (x, y) and its score; with one (keys != nullptr) the image's candidate list gets the key
// (ordered score << 32) | ~(row-major index) at b * cap + rank.  Ranks >= cap are not written.  grid ceil(B H / 4), block 256.
__global__ __launch_bounds__(256) void sp_kp_emit_kernel(const float* __restrict__ score, const unsigned* __restrict__ mask,
                                                         const int* __restrict__ row_off, const int* __restrict__ cu_kp, int64_t rows,
                                                         int H, int W, int Wm, int cap, float* __restrict__ kp, float* __restrict__ sc,
                                                         unsigned long long* __restrict__ keys) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  const int b = (int)(row / H), y = (int)(row % H);
  int base = row_off[row];
  const float* srow = score + row * W;
  const int64_t o0 = keys ? (int64_t)b * cap : (int64_t)cu_kp[b];
  for (int w0 = 0; w0 < Wm && base < cap; w0 += 64) {
    const int w = w0 + lane;
    unsigned m = w < Wm ? mask[row * Wm + w] : 0u;
    const int c = __popc(m);
    int inc = c;
    for (int off = 1; off < 64; off <<= 1) {
      const int v = __shfl_up(inc, off);
      if (lane >= off) inc += v;
    }
    int rank = base + inc - c;
    while (m && rank < cap) {
      const int x = w * 32 + __ffs(m) - 1;
      m &= m - 1;
      const float s = srow[x];
      if (keys) {
        keys[o0 + rank] = ((unsigned long long)kp_ordered(s) << 32) | (unsigned)~(unsigned)(y * W + x);
      } else {
        kp[(o0 + rank) * 2 + 0] = (float)x;
        kp[(o0 + rank) * 2 + 1] = (float)y;
        sc[o0 + rank] = s;
      }
      ++rank;
    }
    base += __shfl(inc, 63);
  }
}

// One block per image.  n = min(found, cap) candidates: n <= k are copied in their row-major order; otherwise the k-th largest key
// is found by a radix select from the top byte down (histograms in LDS), the k keys >= it are gathered into LDS, sorted by a
// bitonic network (descending; the keys are distinct, so the order is total) and written out.
__global__ __launch_bounds__(512) void sp_kp_topk_kernel(const unsigned long long* __restrict__ keys, const int* __restrict__ found,
                                                         const int* __restrict__ cu_kp, int cap, int k, int W, float* __restrict__ kp,
                                                         float* __restrict__ sc) {
  __shared__ unsigned long long sk[KP_MAX_K];
  __shared__ unsigned hist[256];
  __shared__ int s_digit, s_rem, s_cnt;
  const int b = blockIdx.x, t = threadIdx.x;
  const int n = min(found[b], cap);
  const unsigned long long* kb = keys + (int64_t)b * cap;
  const int64_t o0 = cu_kp[b];
  auto put = [&](int i, unsigned long long key) {
    const unsigned idx = ~(unsigned)key;
    kp[(o0 + i) * 2 + 0] = (float)(idx % (unsigned)W);
    kp[(o0 + i) * 2 + 1] = (float)(idx / (unsigned)W);
    sc[o0 + i] = kp_unordered((unsigned)(key >> 32));
  };
  if (n <= k) {
    for (int i = t; i < n; i += 512) put(i, kb[i]);
    return;
  }
  unsigned long long prefix = 0;
  int rem = k;
  for (int shift = 56; shift >= 0; shift -= 8) {
    if (t < 256) hist[t] = 0;
    if (t == 0) s_cnt = 0;
    __syncthreads();
    const unsigned long long himask = shift == 56 ? 0ull : (~0ull << (shift + 8));
    for (int i = t; i < n; i += 512) {
      const unsigned long long key = kb[i];
      if ((key & himask) == prefix) atomicAdd(&hist[(unsigned)(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (t == 0) {       // the bin, from the top, in which the rem-th largest of the matching keys lies
      int left = rem, d = 255;
      for (; d > 0; --d) {
        if ((int)hist[d] >= left) break;
        left -= (int)hist[d];
      }
      s_digit = d;
      s_rem = left;
    }
    __syncthreads();
    prefix |= (unsigned long long)s_digit << shift;
    rem = s_rem;
    __syncthreads();
  }
  // prefix is the k-th largest key: exactly k keys are >= it
  for (int i = t; i < n; i += 512) {
    const unsigned long long key = kb[i];
    if (key >= prefix) {
      const int p = atomicAdd(&s_cnt, 1);
      if (p < KP_MAX_K) sk[p] = key;
    }
  }
  int P = 1;
  while (P < k) P <<= 1;
  for (int i = k + t; i < P; i += 512) sk[i] = 0ull;          // below every real key
  __syncthreads();
  for (int size = 2; size <= P; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int i = t; i < P / 2; i += 512) {
        const int lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
        const bool desc = (lo & size) == 0;
        const unsigned long long a = sk[lo], c = sk[hi];
        if ((a < c) == desc) { sk[lo] = c; sk[hi] = a; }
      }
      __syncthreads();
    }
  for (int i = t; i < k; i += 512) put(i, sk[i]);
}

}  // namespace lt
