// Line segment detector on the device: an LSD / Burns style detector whose every step is independent of any processing order, so the
// device result and the NumPy restatement (tests/line_detector_reference.py) agree exactly up to the region moments and to round-off in the
// final float64 fit.  It fills the surface of the reference's models/line_detector.py:11-28 (LSD.detect / detect_torch) and emits the
// [K,6] rows (startX, startY, endX, endY, lineLength, octave) that linetr_prefilter_batch consumes.  Pixel centres sit at the integers.
//   det_quantise_kernel  octave 0 of a float image: uint8(image * 255), float32 multiply, truncation
//   det_pyramid_kernel   octave o + 1 = separable [1 4 6 4 1] of octave o, reflect-101, (sum + 128) >> 8, even rows and columns
//   det_gradient_kernel  S = [1 2 1] x [1 2 1] * q (reflect-101, kept times 16) on a DET_T x DET_T tile of cells plus halo in LDS; on the
//                        2 x 2 cell: gx, gy, m2 = gx^2 + gy^2, used iff m2 >= grad_threshold, and the two orientation buckets (Burns): A
//                        with boundaries at multiples of 45 degrees, B at 22.5 degrees + multiples of 45, both by integer tests in 64 bit
//   det_label_tile_kernel / det_label_merge_kernel / det_label_flatten_kernel
//                        8-connected components of used cells with the same bucket; a region's label is its smallest linear cell index.
//                        Union-find on parent links that only ever DEcrease: a tile-local pass in LDS, a pass over the cells on tile
//                        borders that links the larger root to the smaller with atomicMin on the global array, and a pass that replaces
//                        every parent by its root.  No thread waits for another thread's write; every loop strictly decreases an index.
//                        In the merge kernel another workgroup (possibly on another XCD) may have just written a label: every read there
//                        is a relaxed agent-scope atomic load, every write an atomicMin.  A stale read would still be a valid ancestor:
//                        the atomicMin's return value is what decides.
//   det_size_kernel / det_vote_kernel / det_moment_kernel / det_extent_kernel
//                        per region: size; votes (a cell votes for partition A iff its A region is at least as large as its B region);
//                        for candidates (size >= min_region_size, 2 * votes > size) n and the six sums of w, wx, wy, wxx, wxy, wyy with
//                        w = floor(sqrt(m2)) as 64-bit integers; the extents of the region along and across its axis as min / max.  A wave
//                        owns 64 consecutive cells, reduces runs of equal keys across its lanes and the run heads issue integer atomics
//                        (min / max of doubles on their order-preserving int64 image): no floating-point atomic sum, the same bits every call.
//   det_assign_kernel    candidates in ascending label order get consecutive slots (one block per image and partition scans the cells)
//   det_fit_kernel       centroid, central second moments, theta = atan2(2 Ixy, Ixx - Iyy) / 2 in float64, one region per thread
//   det_keep_kernel      keep decision (l_max > l_min, density) and the rows, per image octave-major, A before B, ascending label
#pragma once
#include "lt_common.h"

namespace lt {

constexpr int DET_T = 32;                 // a tile is DET_T x DET_T cells, one block of 256 threads, four cells per thread
constexpr int DET_MAX_DIM = 2048;         // the 64-bit moments stay below 2^58: w < 2^14, x^2 < 2^22, n <= 2^22
constexpr int DET_MAX_OCT = 12;
constexpr int DET_MIN_REGION = 4;         // a partition of Nc cells holds at most Nc / 4 candidates: what the candidate tables are sized by
constexpr int DET_DEBUG_LD = 10;          // debug row: octave, partition, label, n, sw, swx, swy, swxx, swxy, swyy

// one octave of one call: extents and where its arrays sit ([..] = per image; both partitions of an image are p * B + b)
struct DetOct {
  int H, W, Hc, Wc;            // pixels, cells = (H - 1) x (W - 1) (0 x 0 when the octave has none)
  int cap;                     // candidate slots per image and partition
  uint8_t* q;                  // [B][H][W]
  int32_t* m2;                 // [B][Nc]
  int8_t* bk;                  // [2B][Nc]   bucket, -1 = unused
  int32_t* raw;                // [2B][Nc]   parent links; from det_assign_kernel on: the candidate slot of a root
  int32_t* lab;                // [2B][Nc]   label = smallest cell index of the region, -1 = unused
  int32_t* size;               // [2B][Nc]   at a root: cells of the region
  int32_t* votes;              // [2B][Nc]   at a root: cells of the region that vote for its partition
  int32_t* c_label;            // [2B][cap]
  long long* c_acc;            // [2B][cap][7]  n, sw, swx, swy, swxx, swxy, swyy
  double* c_geo;               // [2B][cap][4]  cx, cy, dx, dy
  long long* c_ext;            // [2B][cap][4]  l_min, l_max, t_min, t_max as ordered integers
  int32_t* c_count;            // [2B]
};
struct DetPlan { DetOct o[DET_MAX_OCT]; };

__host__ __device__ __forceinline__ int det_reflect(int i, int n) {       // reflect-101 for any i
  if (n == 1) return 0;
  const int period = 2 * n - 2;
  i %= period;
  if (i < 0) i += period;
  return i < n ? i : period - i;
}

// an order-preserving image of a double in the signed 64-bit integers (its own inverse)
__host__ __device__ __forceinline__ long long det_ordered(long long bits) { return bits ^ ((bits >> 63) & 0x7fffffffffffffffLL); }
__device__ __forceinline__ long long det_key(double v) { return det_ordered(__builtin_bit_cast(long long, v)); }
__device__ __forceinline__ double det_unkey(long long k) { return __builtin_bit_cast(double, det_ordered(k)); }

__device__ __forceinline__ void det_buckets(int gx, int gy, int& a, int& b) {
  int k, u, v;
  if (gx > 0 && gy >= 0) { k = 0; u = gx; v = gy; }
  else if (gx <= 0 && gy > 0) { k = 1; u = gy; v = -gx; }
  else if (gx < 0 && gy <= 0) { k = 2; u = -gx; v = -gy; }
  else { k = 3; u = -gy; v = gx; }
  a = 2 * k + (v >= u ? 1 : 0);
  const long long s = (long long)(u + v) * (u + v);
  b = (s < 2LL * u * u ? 2 * k : (s < 2LL * v * v ? 2 * k + 2 : 2 * k + 1)) & 7;
}

__device__ __forceinline__ int det_isqrt(int m2) {
  int w = (int)sqrt((double)m2);
  while ((long long)w * w > m2) --w;
  while ((long long)(w + 1) * (w + 1) <= m2) ++w;
  return w;
}

static __global__ __launch_bounds__(256) void det_quantise_kernel(const float* __restrict__ img, int64_t n, uint8_t* __restrict__ q) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float v = fminf(fmaxf(img[i] * 255.0f, 0.f), 255.f);      // NaN -> 0
  q[i] = (uint8_t)(int)v;
}

// grid (ceil(Wo / 64), ceil(Ho / 4), B), block 256
static __global__ __launch_bounds__(256) void det_pyramid_kernel(const uint8_t* __restrict__ src, int H, int W, uint8_t* __restrict__ dst, int Ho,
                                                                 int Wo) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= Wo || y >= Ho) return;
  const uint8_t* s = src + (int64_t)blockIdx.z * H * W;
  const int k[5] = {1, 4, 6, 4, 1};
  int sum = 0;
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const uint8_t* row = s + (int64_t)det_reflect(2 * y + i - 2, H) * W;
    int r = 0;
#pragma unroll
    for (int j = 0; j < 5; ++j) r += k[j] * row[det_reflect(2 * x + j - 2, W)];
    sum += k[i] * r;
  }
  dst[(int64_t)blockIdx.z * Ho * Wo + (int64_t)y * Wo + x] = (uint8_t)((sum + 128) >> 8);
}

// grid (ceil(Wc / DET_T), ceil(Hc / DET_T), B), block 256.  bkA / bkB: [B][Nc]
static __global__ __launch_bounds__(256) void det_gradient_kernel(const uint8_t* __restrict__ q, int H, int W, int thr, int32_t* __restrict__ m2o,
                                                                  int8_t* __restrict__ bkA, int8_t* __restrict__ bkB) {
  __shared__ int qs[DET_T + 3][DET_T + 4];        // q on the tile's pixels plus one more on every side
  __shared__ int ss[DET_T + 1][DET_T + 2];        // S on the tile's pixels
  const int Hc = H - 1, Wc = W - 1;
  const int x0 = blockIdx.x * DET_T, y0 = blockIdx.y * DET_T;
  const uint8_t* img = q + (int64_t)blockIdx.z * H * W;
  for (int i = threadIdx.x; i < (DET_T + 3) * (DET_T + 3); i += 256) {
    const int r = i / (DET_T + 3), c = i - r * (DET_T + 3);
    qs[r][c] = img[(int64_t)det_reflect(y0 - 1 + r, H) * W + det_reflect(x0 - 1 + c, W)];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < (DET_T + 1) * (DET_T + 1); i += 256) {
    const int r = i / (DET_T + 1), c = i - r * (DET_T + 1);
    ss[r][c] = (qs[r][c] + 2 * qs[r][c + 1] + qs[r][c + 2]) + 2 * (qs[r + 1][c] + 2 * qs[r + 1][c + 1] + qs[r + 1][c + 2]) +
               (qs[r + 2][c] + 2 * qs[r + 2][c + 1] + qs[r + 2][c + 2]);
  }
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.z * Hc * Wc;
  for (int i = threadIdx.x; i < DET_T * DET_T; i += 256) {
    const int r = i / DET_T, c = i % DET_T;
    const int x = x0 + c, y = y0 + r;
    if (x >= Wc || y >= Hc) continue;
    const int s00 = ss[r][c], s01 = ss[r][c + 1], s10 = ss[r + 1][c], s11 = ss[r + 1][c + 1];
    const int gx = s01 + s11 - s00 - s10, gy = s10 + s11 - s00 - s01;
    const int m2 = gx * gx + gy * gy;               // <= 2 * 8160^2 < 2^31
    int a = -1, b = -1;
    if (m2 >= thr) det_buckets(gx, gy, a, b);
    const int64_t at = base + (int64_t)y * Wc + x;
    m2o[at] = m2;
    bkA[at] = (int8_t)a;
    bkB[at] = (int8_t)b;
  }
}

// ---- labelling ---------------------------------------------------------------------------------------------------------------------------

// LDS union-find of one tile.  Links only ever decrease, so find terminates; unite links the larger root to the smaller.
__device__ __forceinline__ int det_lds_find(int* L, int a) {
  for (;;) {
    const int p = __hip_atomic_load(&L[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (p == a) return a;
    a = p;      // p < a
  }
}
__device__ __forceinline__ void det_lds_unite(int* L, int a, int b) {
  for (;;) {
    a = det_lds_find(L, a);
    b = det_lds_find(L, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(&L[a], b);      // a > b
    if (old == a) return;
    a = old;                                   // old < a: a had been linked meanwhile; its former parent still has to meet b
  }
}

// grid (ceil(Wc / DET_T), ceil(Hc / DET_T), images), block 256.  bk / raw: [images][Hc][Wc]
static __global__ __launch_bounds__(256) void det_label_tile_kernel(const int8_t* __restrict__ bk, int Hc, int Wc, int32_t* __restrict__ raw) {
  __shared__ int L[DET_T * DET_T];
  __shared__ int8_t kind[DET_T * DET_T];
  const int x0 = blockIdx.x * DET_T, y0 = blockIdx.y * DET_T;
  const int64_t base = (int64_t)blockIdx.z * Hc * Wc;
  for (int i = threadIdx.x; i < DET_T * DET_T; i += 256) {
    const int x = x0 + i % DET_T, y = y0 + i / DET_T;
    kind[i] = (x < Wc && y < Hc) ? bk[base + (int64_t)y * Wc + x] : (int8_t)-1;
    L[i] = i;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < DET_T * DET_T; i += 256) {
    const int k = kind[i];
    if (k < 0) continue;
    const int r = i / DET_T, c = i % DET_T;
    if (c > 0 && kind[i - 1] == k) det_lds_unite(L, i, i - 1);
    if (r > 0) {
      if (c > 0 && kind[i - DET_T - 1] == k) det_lds_unite(L, i, i - DET_T - 1);
      if (kind[i - DET_T] == k) det_lds_unite(L, i, i - DET_T);
      if (c < DET_T - 1 && kind[i - DET_T + 1] == k) det_lds_unite(L, i, i - DET_T + 1);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < DET_T * DET_T; i += 256) {
    const int x = x0 + i % DET_T, y = y0 + i / DET_T;
    if (x >= Wc || y >= Hc) continue;
    int v = -1;
    if (kind[i] >= 0) {
      const int root = det_lds_find(L, i);      // raster order inside the tile is the image's raster order: the smallest stays the smallest
      v = (y0 + root / DET_T) * Wc + (x0 + root % DET_T);
    }
    raw[base + (int64_t)y * Wc + x] = v;
  }
}

__device__ __forceinline__ int det_glob_find(int32_t* L, int a) {
  for (;;) {
    const int p = __hip_atomic_load(&L[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (p == a) return a;
    a = p;      // p < a
  }
}
__device__ __forceinline__ void det_glob_unite(int32_t* L, int a, int b) {
  for (;;) {
    a = det_glob_find(L, a);
    b = det_glob_find(L, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = __hip_atomic_fetch_min(&L[a], b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old == a) return;
    a = old;
  }
}

// The cells of a tile's top row, left column and right column meet their neighbours W, NW, N, NE in other tiles.
// grid (ceil(Wc / DET_T), ceil(Hc / DET_T), images), block 3 * DET_T
static __global__ __launch_bounds__(3 * DET_T) void det_label_merge_kernel(const int8_t* __restrict__ bk, int Hc, int Wc, int32_t* raw) {
  const int t = threadIdx.x % DET_T, side = threadIdx.x / DET_T;
  const int c = side == 0 ? t : (side == 1 ? 0 : DET_T - 1), r = side == 0 ? 0 : t;
  const int x = blockIdx.x * DET_T + c, y = blockIdx.y * DET_T + r;
  if (x >= Wc || y >= Hc) return;
  const int64_t base = (int64_t)blockIdx.z * Hc * Wc;
  const int8_t* kind = bk + base;
  int32_t* L = raw + base;
  const int me = y * Wc + x;
  const int k = kind[me];
  if (k < 0) return;
  const int dx[4] = {-1, -1, 0, 1}, dy[4] = {0, -1, -1, -1};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int nx = x + dx[j], ny = y + dy[j];
    if (nx < 0 || ny < 0 || nx >= Wc) continue;
    if (nx / DET_T == x / DET_T && ny / DET_T == y / DET_T) continue;       // the tile-local pass has united these
    if (kind[ny * Wc + nx] == k) det_glob_unite(L, me, ny * Wc + nx);
  }
}

// lab = the root of every used cell; size and votes of the image start at zero.  grid (ceil(Nc / 256), images), block 256
static __global__ __launch_bounds__(256) void det_label_flatten_kernel(const int32_t* __restrict__ raw, int Nc, int32_t* __restrict__ lab,
                                                                       int32_t* __restrict__ size, int32_t* __restrict__ votes) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= Nc) return;
  const int64_t base = (int64_t)blockIdx.y * Nc;
  const int32_t* L = raw + base;
  int a = L[i];
  if (a >= 0)
    for (;;) {
      const int p = L[a];
      if (p == a) break;
      a = p;      // p < a
    }
  lab[base + i] = a;
  if (size) { size[base + i] = 0; votes[base + i] = 0; }
}

// ---- per-region reductions -----------------------------------------------------------------------------------------------------------------

// Lanes of a wave hold (key, values) of 64 consecutive cells.  Runs of equal keys are summed (min / max) towards their first lane: after
// the call the lane where `head` is true holds its run's total.  Every lane of the wave must call.
struct DetRun { int id; bool head; };
__device__ __forceinline__ DetRun det_runs(int key) {
  const int lane = threadIdx.x & 63;
  const int prev = __shfl_up(key, 1);
  DetRun r;
  r.head = lane == 0 || prev != key;
  const unsigned long long heads = __ballot(r.head);
  r.id = __popcll(heads & (~0ull >> (63 - lane)));
  return r;
}
enum { DET_ADD = 0, DET_MIN = 1, DET_MAX = 2 };
template <int OP, typename T>
__device__ __forceinline__ T det_run_reduce(const DetRun& run, T v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const T o = __shfl_down(v, off);
    const int id = __shfl_down(run.id, off);
    if (lane + off < 64 && id == run.id) v = OP == DET_ADD ? v + o : (OP == DET_MIN ? (o < v ? o : v) : (o > v ? o : v));
  }
  return v;
}

// grid (ceil(Nc / 256), 2B), block 256
static __global__ __launch_bounds__(256) void det_size_kernel(const int32_t* __restrict__ lab, int Nc, int32_t* size) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int64_t base = (int64_t)blockIdx.y * Nc;
  const int key = i < Nc ? lab[base + i] : -1;
  const DetRun run = det_runs(key);
  const int n = det_run_reduce<DET_ADD>(run, key >= 0 ? 1 : 0);
  if (run.head && key >= 0) atomicAdd(&size[base + key], n);
}

// grid (ceil(Nc / 256), B), block 256
static __global__ __launch_bounds__(256) void det_vote_kernel(const int32_t* __restrict__ lab, const int32_t* __restrict__ size, int Nc, int B,
                                                              int32_t* votes) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int64_t bA = (int64_t)blockIdx.y * Nc, bB = (int64_t)(B + blockIdx.y) * Nc;
  const int la = i < Nc ? lab[bA + i] : -1, lb = i < Nc ? lab[bB + i] : -1;      // a used cell is used in both partitions
  bool forA = false, forB = false;
  if (la >= 0 && lb >= 0) {
    forA = size[bA + la] >= size[bB + lb];
    forB = !forA;
  }
  const DetRun ra = det_runs(la);
  const int na = det_run_reduce<DET_ADD>(ra, forA ? 1 : 0);
  if (ra.head && la >= 0 && na) atomicAdd(&votes[bA + la], na);
  const DetRun rb = det_runs(lb);
  const int nb = det_run_reduce<DET_ADD>(rb, forB ? 1 : 0);
  if (rb.head && lb >= 0 && nb) atomicAdd(&votes[bB + lb], nb);
}

// grid (2B), block 1024: one block walks the cells of one image and partition in raster order
static __global__ __launch_bounds__(1024) void det_assign_kernel(DetOct o, int min_region) {
  __shared__ int wave_n[16];
  __shared__ int s_base;
  const int Nc = o.Hc * o.Wc;
  const int64_t base = (int64_t)blockIdx.x * Nc, cbase = (int64_t)blockIdx.x * o.cap;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) s_base = 0;
  __syncthreads();
  for (int first = 0; first < Nc; first += 1024) {
    const int i = first + threadIdx.x;
    bool cand = false;
    bool root = false;
    if (i < Nc && o.lab[base + i] == i) {
      root = true;
      const int n = o.size[base + i];
      cand = n >= min_region && 2 * o.votes[base + i] > n;
    }
    const unsigned long long m = __ballot(cand);
    if (lane == 0) wave_n[wave] = __popcll(m);
    __syncthreads();
    int before = s_base;
    for (int w = 0; w < wave; ++w) before += wave_n[w];
    int slot = before + __popcll(m & ((1ull << lane) - 1));
    if (cand && slot >= o.cap) { cand = false; }       // cannot happen for min_region >= DET_MIN_REGION; keeps every index inside its table
    if (root) o.raw[base + i] = cand ? slot : -1;
    if (cand) {
      o.c_label[cbase + slot] = i;
      long long* acc = o.c_acc + (cbase + slot) * 7;
#pragma unroll
      for (int k = 0; k < 7; ++k) acc[k] = 0;
      long long* ext = o.c_ext + (cbase + slot) * 4;
      ext[0] = ext[2] = 0x7fffffffffffffffLL;
      ext[1] = ext[3] = -0x7fffffffffffffffLL - 1;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      int total = 0;
      for (int w = 0; w < 16; ++w) total += wave_n[w];
      s_base = min(s_base + total, o.cap);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) o.c_count[blockIdx.x] = s_base;
}

// grid (ceil(Nc / 256), 2B), block 256
static __global__ __launch_bounds__(256) void det_moment_kernel(DetOct o, int B) {
  const int Nc = o.Hc * o.Wc;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int64_t base = (int64_t)blockIdx.y * Nc;
  const int b = blockIdx.y % B;
  int slot = -1;
  long long v[7] = {0, 0, 0, 0, 0, 0, 0};
  if (i < Nc) {
    const int l = o.lab[base + i];
    if (l >= 0) slot = o.raw[base + l];
    if (slot >= 0) {
      const long long w = det_isqrt(o.m2[(int64_t)b * Nc + i]), x = i % o.Wc, y = i / o.Wc;
      v[0] = 1; v[1] = w; v[2] = w * x; v[3] = w * y; v[4] = w * x * x; v[5] = w * x * y; v[6] = w * y * y;
    }
  }
  if (__ballot(slot >= 0) == 0) return;      // the whole wave: most cells belong to no candidate
  const DetRun run = det_runs(slot);
#pragma unroll
  for (int k = 0; k < 7; ++k) v[k] = det_run_reduce<DET_ADD>(run, v[k]);
  if (run.head && slot >= 0) {
    long long* acc = o.c_acc + ((int64_t)blockIdx.y * o.cap + slot) * 7;
#pragma unroll
    for (int k = 0; k < 7; ++k) __hip_atomic_fetch_add(&acc[k], v[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// grid (ceil(cap / 256), 2B), block 256
static __global__ __launch_bounds__(256) void det_fit_kernel(DetOct o) {
  // No FMA contraction here: divisions, products and differences are then the correctly rounded IEEE operations the restatement performs,
  // so the moments of inertia carry the same bits.  For an exactly vertical region Ixy is pure round-off, and its SIGN decides
  // which end of the line is the start.
#pragma clang fp contract(off)
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= o.c_count[blockIdx.y]) return;
  const int64_t at = (int64_t)blockIdx.y * o.cap + s;
  const long long* a = o.c_acc + at * 7;
  const double sw = (double)a[1];
  const double cx = (double)a[2] / sw, cy = (double)a[3] / sw;
  const double ixx = (double)a[4] / sw - cx * cx, ixy = (double)a[5] / sw - cx * cy, iyy = (double)a[6] / sw - cy * cy;
  const double theta = 0.5 * atan2(2.0 * ixy, ixx - iyy);
  double* g = o.c_geo + at * 4;
  g[0] = cx; g[1] = cy; g[2] = cos(theta); g[3] = sin(theta);
}

// grid (ceil(Nc / 256), 2B), block 256
static __global__ __launch_bounds__(256) void det_extent_kernel(DetOct o) {
  const int Nc = o.Hc * o.Wc;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int64_t base = (int64_t)blockIdx.y * Nc;
  int slot = -1;
  long long l = 0, t = 0;
  if (i < Nc) {
    const int lb = o.lab[base + i];
    if (lb >= 0) slot = o.raw[base + lb];
    if (slot >= 0) {
      const double* g = o.c_geo + ((int64_t)blockIdx.y * o.cap + slot) * 4;
      const double px = (double)(i % o.Wc) - g[0], py = (double)(i / o.Wc) - g[1];
      l = det_key(px * g[2] + py * g[3]);
      t = det_key(py * g[2] - px * g[3]);
    }
  }
  if (__ballot(slot >= 0) == 0) return;      // the whole wave
  const DetRun run = det_runs(slot);
  const long long lmin = det_run_reduce<DET_MIN>(run, l), lmax = det_run_reduce<DET_MAX>(run, l);
  const long long tmin = det_run_reduce<DET_MIN>(run, t), tmax = det_run_reduce<DET_MAX>(run, t);
  if (run.head && slot >= 0) {
    long long* e = o.c_ext + ((int64_t)blockIdx.y * o.cap + slot) * 4;
    __hip_atomic_fetch_min(&e[0], lmin, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_max(&e[1], lmax, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_min(&e[2], tmin, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_max(&e[3], tmax, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// grid (B), block 256: the rows of one image in their order; counts [B][n_oct] hold the true numbers whatever the capacity
static __global__ __launch_bounds__(256) void det_keep_kernel(DetPlan plan, int n_oct, int B, double density, int capacity, double* __restrict__ rows,
                                                              int32_t* __restrict__ counts, long long* __restrict__ debug) {
  __shared__ int wave_n[4];
  __shared__ int s_at;
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) s_at = 0;
  __syncthreads();
  for (int oc = 0; oc < n_oct; ++oc) {
    const DetOct& o = plan.o[oc];
    const int at_octave = s_at;
    if (o.Hc > 0 && o.Wc > 0)
      for (int p = 0; p < 2; ++p) {
        const int img = p * B + b;
        const int n = o.c_count[img];
        const int64_t cbase = (int64_t)img * o.cap;
        for (int first = 0; first < n; first += 256) {
          const int s = first + threadIdx.x;
          bool keep = false;
          double lmin = 0, lmax = 0;
          if (s < n) {
            const long long* e = o.c_ext + (cbase + s) * 4;
            lmin = det_unkey(e[0]); lmax = det_unkey(e[1]);
            const double tmin = det_unkey(e[2]), tmax = det_unkey(e[3]);
            const double cells = (double)o.c_acc[(cbase + s) * 7];
            keep = lmax > lmin && !(cells / ((lmax - lmin + 1.0) * (tmax - tmin + 1.0)) < density);
          }
          const unsigned long long m = __ballot(keep);
          if (lane == 0) wave_n[wave] = __popcll(m);
          __syncthreads();
          int row = s_at;
          for (int w = 0; w < wave; ++w) row += wave_n[w];
          row += __popcll(m & ((1ull << lane) - 1));
          if (keep && row < capacity) {
            const double* g = o.c_geo + (cbase + s) * 4;
            const double scale = (double)(1 << oc);
            double* r = rows + ((int64_t)b * capacity + row) * 6;
            r[0] = (g[0] + lmin * g[2] + 0.5) * scale;
            r[1] = (g[1] + lmin * g[3] + 0.5) * scale;
            r[2] = (g[0] + lmax * g[2] + 0.5) * scale;
            r[3] = (g[1] + lmax * g[3] + 0.5) * scale;
            r[4] = lmax - lmin;
            r[5] = (double)oc;
            if (debug) {
              long long* d = debug + ((int64_t)b * capacity + row) * DET_DEBUG_LD;
              const long long* a = o.c_acc + (cbase + s) * 7;
              d[0] = oc; d[1] = p; d[2] = o.c_label[cbase + s];
#pragma unroll
              for (int k = 0; k < 7; ++k) d[3 + k] = a[k];
            }
          }
          __syncthreads();
          if (threadIdx.x == 0) s_at += wave_n[0] + wave_n[1] + wave_n[2] + wave_n[3];
          __syncthreads();
        }
      }
    if (threadIdx.x == 0) counts[b * n_oct + oc] = s_at - at_octave;
    __syncthreads();
  }
}

}  // namespace lt
