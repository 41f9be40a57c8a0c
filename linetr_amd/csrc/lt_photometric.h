// Photometric augmentation on the device: the distortions of the reference's dataset builder (dataloaders/build_homography_dataset.py:105-121,
// 154-158; dataloaders/utils/photometric.py ImgAugTransform followed by customizedTransform) for batches of float32 grey images, seeded and
// deterministic.  Values are grey LEVELS 0..255 held as float; quantise(v) = rint(min(max(v, 0), 255)), half to even.  The stages, in this
// order, each enabled per image by its bit of LinetrPhotoParams.stages (a disabled stage passes its input on):
//   0 input       level = quantise(255 x), the product exact in float64 (the reference truncates a float64 quotient; both give the same
//                 level for the 256 values k / 255)
//   1 brightness  quantise(level + d), integer d
//   2 contrast    quantise(127 + alpha (level - 127)), float64, one rounding per operation, no contraction
//   3 noise       quantise(level + sigma z), float64; z by Box-Muller: u1, u2 = the two 53-bit uniforms of one Philox call,
//                 r = sqrt(-2 log(1 - u1)), z = r cos(2 pi u2) for the even pixel of a pair and r sin(2 pi u2) for the odd one
//   4 impulse     a pixel whose 32-bit word is below thr becomes 255 if bit 0 of its polarity word is set, else 0
//   5 motion      correlation with the image's K x K float32 kernel (K in 1, 3, 5, 7; row-major in weights[0 .. K K)), border reflect-101:
//                 acc = 0, then acc = acc + w[ky][kx] * level(y + ky - K / 2, x + kx - K / 2) for ky ascending, kx ascending inside, every
//                 product and sum rounded to float32 (no contraction); then quantise
//   6 blur        separable Gaussian of odd ksize <= 351: taps exp(-(k - r)^2 / (2 sigma^2)), r = ksize / 2, sigma as given or
//                 0.3 ((ksize - 1) / 2 - 1) + 0.8 when 0, normalised in float64 and rounded to float32 once; rows first, then columns,
//                 each a direct float32 sum of tap * value over k ascending (fused multiply-adds), reflect-101; then quantise
//   7 shade       mask = 255 inside any of the image's ellipses, ((dx c + dy s) / ax)^2 + ((dy c - dx s) / ay)^2 <= 1 in float64 with
//                 dx = x - cx, dy = y - cy, else 0; m = the mask under the stage-6 blur at shade_ksize (sigma 0), NOT quantised;
//                 shaded = min(max(level (1 - t m / 255), 0), 255) in float64; output shaded / 255, or floor(shaded) / 255 with
//                 quantise_out (the builder's (... * 255).astype('uint8')), the quotient taken in float64 and rounded to float32 once
// reflect-101 of an index is the repeated reflection of period 2 (n - 1) (n = 1: always 0), whatever the radius.
//
// Per-pixel randomness is Philox4x32-10 (lt_common.h) with key = (seed, image index) and counter = (x / 4, y, draw, 0): one call yields the
// four words of the pixels 4 (x / 4) .. 4 (x / 4) + 3 of row y.  draw 0: the normals of pixels 0, 1 (u1 from words 0, 1; u2 from words 2, 3);
// draw 1: those of pixels 2, 3; draw 2: the impulse words; draw 3: the polarity words.  A pixel's bits depend on (seed, image, x, y) alone:
// not on the launch geometry, the chunking of a batch or the stages of other images; halo pixels are recomputed, not exchanged.  The host
// sampler (linetr_photometric_sample) draws with counter = (n, 0, 0, 1), which no pixel uses.
//
// Deviations from imgaug / OpenCV: salt-and-pepper values are 0 / 255, not a Beta draw; the ellipse test is the analytic form above, not
// cv2.ellipse's polygon; stage 0 rounds; the Gaussian taps follow the formula for every ksize (OpenCV has tables for ksize <= 7); the motion
// kernel is an anti-aliased line through the centre (linetr_photometric_sample), not imgaug's rotated matrix.
//
// Launches of a batch: one small carrier launch per PH_CARRY images (their parameters travel in the kernel's arguments into the workspace and
// the Gaussian taps are made there), then
//   photo_point_kernel   stages 0-5: the point stages of a PH_TW x PH_TH tile plus the motion halo go to LDS, the correlation runs from LDS
//   photo_row_kernel     the row pass of a blur over a PH_BW x PH_BR strip plus a halo of the radius in LDS; for the shade the strip is
//                        filled with the analytic mask of the ellipses that reach its rows; the mask never reaches memory
//   photo_col_kernel     the column pass on PH_CW x PH_CH pixels, 16 consecutive rows per thread in registers, and the epilogue: the
//                        quantisation of stage 6 or the shade and the output
// Plain loads and stores, no atomics: the same call gives the same bits.  Inputs must be finite: the blur passes multiply values next to a
// window by zero taps, so a non-finite value spreads beyond its window.
#pragma once
#include "lt_common.h"

namespace lt {

constexpr int PH_TW = 64, PH_TH = 32, PH_HALO = 3;                 // point kernel: tile and the halo of K = 7
constexpr int PH_LG = PH_TW / 4 + 2, PH_LW = PH_LG * 4, PH_LH = PH_TH + 2 * PH_HALO;      // LDS tile in 4-pixel groups: one group of halo each side
constexpr int PH_MAX_R = LINETR_PHOTO_MAX_KSIZE / 2, PH_TAPS = 352;  // blur radius limit; floats per tap row (zero beyond ksize)
constexpr int PH_BW = 256, PH_BR = 8;                              // row pass: columns x rows of a block (a thread: 4 columns x 2 rows)
constexpr int PH_RLW = PH_BW + 2 * PH_MAX_R + 10;                  // LDS row: strip, halo, 8 zeros; a multiple of 4 floats
constexpr int PH_RTP = 3 + PH_TAPS + 13;                           // LDS taps of the row pass: 3 zeros, the taps, zeros up to index 367
static_assert(PH_RLW % 4 == 0 && PH_RTP % 4 == 0 && PH_RTP >= LINETR_PHOTO_MAX_KSIZE + 3 + 8, "16-byte reads of the row pass");
constexpr int PH_CW = 64, PH_CRY = 16, PH_CH = 4 * PH_CRY;         // column pass: columns x rows per thread, 4 row groups per block
constexpr int PH_CTP = PH_CRY - 1 + PH_TAPS + 2 * PH_CRY + 1;       // LDS taps of the column pass: 15 zeros, the taps, zeros up to index 399
static_assert(PH_CTP % 4 == 0 && PH_CTP >= 2 * PH_MAX_R + PH_CRY + 2 * PH_CRY, "16-byte reads of the column pass");
constexpr int PH_CARRY = 3;                                        // images per carrier launch (3 x 1224 bytes of the 4 KB of arguments)
struct PhotoChunk { LinetrPhotoParams p[PH_CARRY]; };
static_assert(sizeof(PhotoChunk) <= 4096 - 64, "the carrier's arguments");

__host__ __device__ __forceinline__ int reflect101(int v, int n) {
  if ((unsigned)v < (unsigned)n) return v;
  if (n == 1) return 0;
  const int period = 2 * (n - 1);
  v %= period;
  if (v < 0) v += period;
  return v < n ? v : period - v;
}
__host__ __device__ __forceinline__ double photo_u01(uint32_t hi, uint32_t lo) {
  return ((double)(hi >> 5) * 67108864.0 + (double)(lo >> 6)) / 9007199254740992.0;
}
__device__ __forceinline__ double photo_quantise(double v) { return rint(fmin(fmax(v, 0.0), 255.0)); }

// grid (images of this launch, 2), block 64: row 0 copies the parameters and makes the taps of stage 6, row 1 the taps of the shade
static __global__ __launch_bounds__(64) void photo_carrier_kernel(const PhotoChunk c, int first, LinetrPhotoParams* __restrict__ table,
                                                                  float* __restrict__ taps) {
  __shared__ double e[2 * PH_MAX_R + 1];
  __shared__ double total;
  const int i = blockIdx.x, which = blockIdx.y, tid = threadIdx.x;
  const LinetrPhotoParams* p = &c.p[i];
  if (which == 0) {
    const uint32_t* s = reinterpret_cast<const uint32_t*>(p);
    uint32_t* d = reinterpret_cast<uint32_t*>(table + first + i);
    for (int w = tid; w < (int)(sizeof(LinetrPhotoParams) / 4); w += 64) d[w] = s[w];
  }
  const bool on = p->stages & (which ? LINETR_PHOTO_SHADE : LINETR_PHOTO_BLUR);
  const int ksize = on ? (which ? p->shade_ksize : p->blur_ksize) : 1, r = ksize / 2;
  double sigma = on && !which ? p->blur_sigma : 0.0;
  if (sigma == 0.0) sigma = 0.3 * ((ksize - 1) / 2.0 - 1.0) + 0.8;
  const double scale = -1.0 / (2.0 * sigma * sigma);
  for (int k = tid; k < ksize; k += 64) e[k] = exp((double)((k - r) * (k - r)) * scale);
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    for (int k = 0; k < ksize; ++k) s += e[k];
    total = s;
  }
  __syncthreads();
  float* t = taps + ((int64_t)(first + i) * 2 + which) * PH_TAPS;
  for (int k = tid; k < PH_TAPS; k += 64) t[k] = k < ksize ? (float)(e[k] / total) : 0.f;
}

// stages 0-4 of the pixels 4 xg .. 4 xg + 3 of row y (v: their inputs)
__device__ __forceinline__ void photo_point_stages(const float (&v)[4], int xg, int y, int stages, int d, double alpha, double sigma,
                                                   uint32_t thr, uint32_t seed, uint32_t image, float (&out)[4]) {
#pragma clang fp contract(off)
  double l[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) l[j] = photo_quantise(255.0 * (double)v[j]);
  if (stages & LINETR_PHOTO_BRIGHTNESS) {
#pragma unroll
    for (int j = 0; j < 4; ++j) l[j] = photo_quantise(l[j] + (double)d);
  }
  if (stages & LINETR_PHOTO_CONTRAST) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const double scaled = alpha * (l[j] - 127.0);
      l[j] = photo_quantise(127.0 + scaled);
    }
  }
  if (stages & LINETR_PHOTO_NOISE) {
#pragma unroll
    for (int pair = 0; pair < 2; ++pair) {
      uint32_t w[4];
      philox4x32_10((uint32_t)xg, (uint32_t)y, (uint32_t)pair, 0u, seed, image, w);
      const double u1 = photo_u01(w[0], w[1]), u2 = photo_u01(w[2], w[3]);
      const double r = sqrt(-2.0 * log(1.0 - u1)), th = 6.283185307179586 * u2;
      double sn, cs;
      sincos(th, &sn, &cs);
      const double z0 = r * cs, z1 = r * sn;
      const double n0 = sigma * z0, n1 = sigma * z1;
      l[2 * pair] = photo_quantise(l[2 * pair] + n0);
      l[2 * pair + 1] = photo_quantise(l[2 * pair + 1] + n1);
    }
  }
  if (stages & LINETR_PHOTO_IMPULSE) {
    uint32_t a[4], pol[4];
    philox4x32_10((uint32_t)xg, (uint32_t)y, 2u, 0u, seed, image, a);
    philox4x32_10((uint32_t)xg, (uint32_t)y, 3u, 0u, seed, image, pol);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (a[j] < thr) l[j] = (pol[j] & 1u) ? 255.0 : 0.0;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) out[j] = (float)l[j];
}

// grid (ceil(W / PH_TW), ceil(H / PH_TH), B), block 256.  src / lev: [B][H][W]; image = first + blockIdx.z keys the generator.
static __global__ __launch_bounds__(256) void photo_point_kernel(const float* __restrict__ src, const LinetrPhotoParams* __restrict__ table,
                                                                 uint32_t seed, int first, int H, int W, int vec, float* __restrict__ lev) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) float tile[PH_LH][PH_LW];
  __shared__ float wk[LINETR_PHOTO_MAX_K * LINETR_PHOTO_MAX_K];
  const int tid = threadIdx.x, b = blockIdx.z;
  const LinetrPhotoParams* p = table + b;
  const int stages = p->stages, d = p->d;
  const double alpha = p->alpha, sigma = p->sigma;
  const uint32_t thr = p->thr;
  const bool motion = stages & LINETR_PHOTO_MOTION;
  const int K = motion ? p->K : 1, r = K / 2;
  const int x0 = blockIdx.x * PH_TW, y0 = blockIdx.y * PH_TH;
  if (tid < LINETR_PHOTO_MAX_K * LINETR_PHOTO_MAX_K) wk[tid] = p->weights[tid];
  const float* plane = src + (int64_t)b * H * W;
  // In-image pixels of rows y0 - 3 .. y0 + PH_TH + 2 and groups x0 / 4 - 1 .. x0 / 4 + PH_TW / 4.  A reflected coordinate of the window of
  // a pixel of this tile lies inside the image and inside that range, so the correlation reads nothing that was not written here.
  for (int i = tid; i < PH_LH * PH_LG; i += 256) {
    const int rr = i / PH_LG, g = i - rr * PH_LG;
    const int y = y0 - PH_HALO + rr, xg = x0 / 4 - 1 + g;
    if (y < 0 || y >= H || xg < 0 || 4 * xg >= W) continue;
    if (r == 0 && (rr < PH_HALO || rr >= PH_HALO + PH_TH || g == 0 || g == PH_LG - 1)) continue;     // no halo needed
    const float* s = plane + (int64_t)y * W + 4 * xg;
    float v[4], o[4];
    if (vec) {
      const f32x4 q = *reinterpret_cast<const f32x4*>(s);
      v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = 4 * xg + j < W ? s[j] : 0.f;
    }
    photo_point_stages(v, xg, y, stages, d, alpha, sigma, thr, seed, (uint32_t)(first + b), o);
    *reinterpret_cast<f32x4*>(&tile[rr][4 * g]) = f32x4{o[0], o[1], o[2], o[3]};
  }
  __syncthreads();
  float* out = lev + (int64_t)b * H * W;
  for (int o = tid; o < PH_TH * PH_TW; o += 256) {
    const int ty = o / PH_TW, tx = o - ty * PH_TW;
    const int x = x0 + tx, y = y0 + ty;
    if (x >= W || y >= H) continue;
    float res = tile[ty + PH_HALO][tx + 4];
    if (motion) {
      float acc = 0.f;
      for (int ky = 0; ky < K; ++ky) {
        const int ly = reflect101(y + ky - r, H) - (y0 - PH_HALO);
        for (int kx = 0; kx < K; ++kx) {
          const int lx = reflect101(x + kx - r, W) - (x0 - 4);
          const float prod = wk[ky * K + kx] * tile[ly][lx];
          acc = acc + prod;
        }
      }
      res = rintf(fminf(fmaxf(acc, 0.f), 255.f));
    }
    out[(int64_t)y * W + x] = res;
  }
}

// 255 inside any ellipse, else 0.  el: n x (cx, cy, ax, ay, c, s, reach, -) in LDS, reach = max(ax, ay) + 1.  An ellipse whose centre is
// further than its reach in x or in y cannot contain the pixel ((u / ax)^2 + (v / ay)^2 >= (u^2 + v^2) / max(ax, ay)^2) and is skipped
// without the float64 form.
constexpr int PH_EL = 8;
__device__ __forceinline__ float photo_mask_at(const double* el, int n, int x, int y) {
#pragma clang fp contract(off)
  for (int e = 0; e < n; ++e) {
    const double* q = el + PH_EL * e;
    const double dx = (double)x - q[0], dy = (double)y - q[1];
    if (fabs(dx) > q[6] || fabs(dy) > q[6]) continue;
    const double a = (dx * q[4] + dy * q[5]) / q[2], bq = (dy * q[4] - dx * q[5]) / q[3];
    if (a * a + bq * bq <= 1.0) return 255.f;
  }
  return 0.f;
}

// The row pass.  grid (ceil(W / PH_BW), ceil(H / PH_BR), planes), block 256; plane = image * C + channel.  An image without `need` in its
// stages is left alone.  MASK: the strip is filled from the image's ellipses instead of src (C = 1).
template <bool MASK>
static __global__ __launch_bounds__(256) void photo_row_kernel(const float* __restrict__ src, const LinetrPhotoParams* __restrict__ table,
                                                               const float* __restrict__ taps, int which, int need, int C, int H, int W,
                                                               float* __restrict__ rowsum) {
  __shared__ __attribute__((aligned(16))) float rows[PH_BR][PH_RLW];
  __shared__ __attribute__((aligned(16))) float tp[PH_RTP];           // tp[3 + k] = tap k, zeros around
  __shared__ double el[MASK ? LINETR_PHOTO_MAX_ELLIPSES * PH_EL : 1];
  __shared__ int n_kept;
  const int tid = threadIdx.x, pl = blockIdx.z, img = pl / C;
  const LinetrPhotoParams* p = table + img;
  if (!(p->stages & need)) return;
  const int ksize = which ? p->shade_ksize : p->blur_ksize, r = ksize / 2;
  const int x0 = blockIdx.x * PH_BW, y0 = blockIdx.y * PH_BR;
  int n_el = 0;
  if (MASK) {
    // the ellipses that can reach a row of this strip, in their order (wave 0 compacts them by a ballot); the others are never looked at
    if (tid < WAVE) {
      const bool have = tid < p->n_ellipses;
      const double cy = have ? p->ellipse[tid][1] : 0.0;
      const double reach = have ? fmax(p->ellipse[tid][2], p->ellipse[tid][3]) + 1.0 : 0.0;
      const bool keep = have && cy + reach >= (double)y0 && cy - reach <= (double)(y0 + PH_BR - 1);
      const unsigned long long m = __ballot(keep);
      if (keep) {
        double* q = el + PH_EL * __popcll(m & ((1ull << tid) - 1ull));
#pragma unroll
        for (int j = 0; j < 6; ++j) q[j] = p->ellipse[tid][j];
        q[6] = reach;
      }
      if (tid == 0) n_kept = __popcll(m);
    }
    __syncthreads();
    n_el = n_kept;
  }
  const float* tg = taps + ((int64_t)img * 2 + which) * PH_TAPS;
  for (int k = tid; k < PH_RTP; k += 256) tp[k] = (k >= 3 && k < 3 + PH_TAPS) ? tg[k - 3] : 0.f;
  const int64_t base = (int64_t)pl * H * W;
  // the strip plus its halo, and 8 zeros behind it: the last group of four values a thread reads may lie beyond the window (under zero taps)
  const int lw = PH_BW + 2 * r, lwp = lw + 8;
  for (int i = tid; i < PH_BR * lwp; i += 256) {
    const int rr = i / lwp, cc = i - rr * lwp;
    const int y = y0 + rr;
    float v = 0.f;
    if (y < H && cc < lw) {
      const int x = reflect101(x0 - r + cc, W);
      v = MASK ? photo_mask_at(el, n_el, x, y) : src[base + (int64_t)y * W + x];
    }
    rows[rr][cc] = v;
  }
  __syncthreads();
  // A thread owns four adjacent columns of two rows.  The value at offset m from its first column meets tap m - j in column j, so four
  // values (one 16-byte read) and the seven taps m4 - 3 .. m4 + 3 (two 16-byte broadcast reads) feed 16 multiply-adds; every column still
  // sums its taps in ascending order, the taps outside 0 .. ksize - 1 being zeros.
  const int c0 = 4 * (tid & 63), ra = 2 * (tid >> 6);
  const int x = x0 + c0;
  if (x >= W) return;
  float acc[2][4];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[a][j] = 0.f;
  for (int m4 = 0; m4 < ksize + 3; m4 += 4) {
    const f32x4 ta = *reinterpret_cast<const f32x4*>(&tp[m4]), tb = *reinterpret_cast<const f32x4*>(&tp[m4 + 4]);
    const float t[8] = {ta[0], ta[1], ta[2], ta[3], tb[0], tb[1], tb[2], tb[3]};          // t[e] = tap m4 - 3 + e
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(&rows[ra + a][c0 + m4]);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[a][j] = fmaf(t[3 + i - j], v[i], acc[a][j]);
    }
  }
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    const int y = y0 + ra + a;
    if (y >= H) continue;
    float* o = rowsum + base + (int64_t)y * W + x;
    if (W % 4 == 0) *reinterpret_cast<f32x4*>(o) = f32x4{acc[a][0], acc[a][1], acc[a][2], acc[a][3]};
    else
      for (int j = 0; j < 4 && x + j < W; ++j) o[j] = acc[a][j];
  }
}

// The column pass and its epilogue.  grid (ceil(W / PH_CW), ceil(H / PH_CH), planes), block 256 = PH_CW columns x 4 groups of PH_CRY rows.
// MODE 0: out = the blur; 1: out = quantise(blur); an image without `need` copies `lev` (the pass's source plane).
// MODE 2: out = shade(lev, blur) / 255; an image without `need` gives lev / 255.
template <int MODE>
static __global__ __launch_bounds__(256) void photo_col_kernel(const float* __restrict__ rowsum, const float* __restrict__ lev,
                                                               const LinetrPhotoParams* __restrict__ table, const float* __restrict__ taps,
                                                               int which, int need, int C, int H, int W, int quantise_out,
                                                               float* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) float tp[PH_CTP];          // taps between zeros: tp[PH_CRY - 1 + k] = tap k
  const int tid = threadIdx.x, pl = blockIdx.z, img = pl / C;
  const LinetrPhotoParams* p = table + img;
  const bool on = p->stages & need;
  const int ksize = on ? (which ? p->shade_ksize : p->blur_ksize) : 1, r = ksize / 2;
  const double t = p->t;
  const float* tg = taps + ((int64_t)img * 2 + which) * PH_TAPS;
  for (int k = tid; k < PH_CTP; k += 256) tp[k] = (k >= PH_CRY - 1 && k < PH_CRY - 1 + PH_TAPS) ? tg[k - (PH_CRY - 1)] : 0.f;
  __syncthreads();
  const int x = blockIdx.x * PH_CW + (tid & (PH_CW - 1));
  const int yb = blockIdx.y * PH_CH + (tid / PH_CW) * PH_CRY;
  if (x >= W || yb >= H) return;
  const int64_t base = (int64_t)pl * H * W;
  float acc[PH_CRY];
#pragma unroll
  for (int i = 0; i < PH_CRY; ++i) acc[i] = 0.f;
  if (on) {
    // Row yb - r + jj meets tap jj - i in output row i.  16 rows at a time: their 31 taps jj0 - 15 .. jj0 + 15 come from LDS in eight 16-byte
    // broadcast reads and stay in registers for 256 multiply-adds; the taps outside 0 .. ksize - 1 are zeros, so the rows beyond
    // PH_CRY + 2 r - 1 that the last group touches add nothing, and every output sums its taps in ascending order.
    for (int jj0 = 0; jj0 < PH_CRY + 2 * r; jj0 += PH_CRY) {
      float tb[2 * PH_CRY];
#pragma unroll
      for (int e = 0; e < 2 * PH_CRY; e += 4) {
        const f32x4 q = *reinterpret_cast<const f32x4*>(&tp[jj0 + e]);
        tb[e] = q[0]; tb[e + 1] = q[1]; tb[e + 2] = q[2]; tb[e + 3] = q[3];
      }
#pragma unroll
      for (int u = 0; u < PH_CRY; ++u) {
        const float v = rowsum[base + (int64_t)reflect101(yb - r + jj0 + u, H) * W + x];
#pragma unroll
        for (int i = 0; i < PH_CRY; ++i) acc[i] = fmaf(tb[PH_CRY - 1 + u - i], v, acc[i]);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < PH_CRY; ++i) {
    const int y = yb + i;
    if (y >= H) break;
    const int64_t at = base + (int64_t)y * W + x;
    float res;
    if (MODE == 2) {
      double shaded = (double)lev[at];
      if (on) {
        const double tm = t * (double)acc[i];
        const double f = 1.0 - tm / 255.0;
        shaded = fmin(fmax(shaded * f, 0.0), 255.0);
        if (quantise_out) shaded = floor(shaded);
      }
      res = (float)(shaded / 255.0);
    } else if (!on) {
      res = lev[at];
    } else {
      res = MODE == 1 ? rintf(fminf(fmaxf(acc[i], 0.f), 255.f)) : acc[i];
    }
    out[at] = res;
  }
}

}  // namespace lt
