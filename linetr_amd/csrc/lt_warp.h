// Homography views on the device: the step of the reference's dataset builder between "an image" and "a training pair"
// (dataloaders/build_homography_dataset.py:164-167 warps the image, :179-184 builds and erodes the valid mask of the view), and the
// torch recipe of dataloaders/utils/utils.py:317-351 (inv_warp_image_batch) / :677-704 (compute_valid_mask) without its [B,H,W,2] grid.
//   warp_kernel    dst[b, c, y, x] = src[b, c] sampled at M_b (x, y, 1), zero padding, bilinear or nearest (F.grid_sample with
//                  align_corners=True read in pixel units), and valid[b, y, x] = "the nearest source pixel lies inside the image".
//                  The source position is computed ONCE per pixel in float64 (one reciprocal, two products) and clamped to
//                  [-2, extent + 1] BEFORE any conversion to an integer: every position outside (-1, extent) has all its taps
//                  outside the image whatever its value, so the clamp changes no result and no index can leave [-2, extent + 2].
//                  A non-finite position (w' == 0, overflow) has no tap at all.  A tap that does not exist is loaded from offset 0 of
//                  the plane and discarded by a select, so every address is inside the tensor and the loads need no branch.
//                  Block = WARP_TW x WARP_TH output pixels (64 x 16), a thread owns WARP_PX = 4 consecutive x of one row, a wave 64 x 4
//                  pixels: under a rotation the taps of one wave instruction stay inside a patch of about 64 x 64 source pixels.  The
//                  channel loop runs inside the thread over positions and weights held in registers.  16-byte stores to dst and one
//                  4-byte store to valid where the row allows (W % 4 == 0 and aligned bases), scalar stores otherwise.
//   erode_kernel   binary erosion by the (2 r + 1)^2 square of ones, pixels outside the image count as set (cv2.erode's default border,
//                  scipy.ndimage.binary_erosion(border_value=1)): a ERODE_TW x ERODE_TH tile (64 x 32) plus a halo of r is normalised to 0 / 1
//                  into LDS, a horizontal AND over 2 r + 1 columns and a vertical AND over 2 r + 1 rows follow (the minimum of 0 / 1
//                  values), the vertical one on four pixels per 32-bit word.
// Plain loads and stores, no atomics: the same call gives the same bits.
#pragma once
#include "lt_common.h"

namespace lt {

constexpr int WARP_TW = 64, WARP_TH = 16, WARP_PX = 4;      // block 256 = (WARP_TW / WARP_PX) x WARP_TH threads
constexpr int WARP_CHUNK = 32;                               // images per launch: their matrices travel in the kernel's arguments
struct WarpMats { double m[WARP_CHUNK][9]; };

// the source position of one destination pixel and what both sampling modes need from it
struct WarpTap {
  int x0, y0;          // floor of the (clamped) position: the bilinear taps are x0, x0 + 1 / y0, y0 + 1
  int xn, yn;          // the nearest pixel (half to even)
  float w00, w01, w10, w11;
  bool finite;
};

__device__ __forceinline__ WarpTap warp_tap(const double* __restrict__ m, int x, int y, int H, int W) {
  const double dx = (double)x, dy = (double)y;
  const double xs = m[0] * dx + m[1] * dy + m[2];
  const double ys = m[3] * dx + m[4] * dy + m[5];
  const double ws = m[6] * dx + m[7] * dy + m[8];
  const double inv = 1.0 / ws;
  double sx = xs * inv, sy = ys * inv;
  WarpTap t;
  t.finite = isfinite(sx) && isfinite(sy);
  if (!t.finite) sx = sy = -2.0;
  sx = fmin(fmax(sx, -2.0), (double)W + 1.0);      // before any integer conversion
  sy = fmin(fmax(sy, -2.0), (double)H + 1.0);
  const double fx0 = floor(sx), fy0 = floor(sy);
  t.x0 = (int)fx0;
  t.y0 = (int)fy0;
  t.xn = (int)rint(sx);
  t.yn = (int)rint(sy);
  const double fx = sx - fx0, fy = sy - fy0;
  t.w00 = (float)((1.0 - fx) * (1.0 - fy));
  t.w01 = (float)(fx * (1.0 - fy));
  t.w10 = (float)((1.0 - fx) * fy);
  t.w11 = (float)(fx * fy);
  return t;
}

// grid (ceil(W / WARP_TW), ceil(H / WARP_TH), images of this launch), block 256
template <int MODE>
static __global__ __launch_bounds__(256) void warp_kernel(const float* __restrict__ src, const WarpMats mats, int first, int C, int H, int W,
                                                          int vec, float* __restrict__ dst, uint8_t* __restrict__ valid) {
  const int tx = threadIdx.x & (WARP_TW / WARP_PX - 1), ty = threadIdx.x / (WARP_TW / WARP_PX);
  const int x = blockIdx.x * WARP_TW + tx * WARP_PX, y = blockIdx.y * WARP_TH + ty;
  if (x >= W || y >= H) return;
  const int b = first + (int)blockIdx.z;
  const double* m = mats.m[blockIdx.z];
  const int64_t plane = (int64_t)H * W;
  const int n = W - x < WARP_PX ? W - x : WARP_PX;     // pixels of this thread inside the row
  // Plane offsets of the taps and one bit per tap that exists.  A tap that does not exist keeps offset 0, the plane's first pixel:
  // the channel loop below loads all its taps unconditionally (back to back, nothing waits on a branch) and selects afterwards, so
  // whatever that pixel holds never reaches a result.
  int off[WARP_PX][4];
  float wt[WARP_PX][4];
  uint32_t vbits = 0, taps = 0;
#pragma unroll
  for (int i = 0; i < WARP_PX; ++i) {
    off[i][0] = off[i][1] = off[i][2] = off[i][3] = 0;
    wt[i][0] = wt[i][1] = wt[i][2] = wt[i][3] = 0.f;
    if (i >= n) continue;
    const WarpTap t = warp_tap(m, x + i, y, H, W);
    if (!t.finite) continue;
    const bool near_in = t.xn >= 0 && t.xn < W && t.yn >= 0 && t.yn < H;
    if (near_in) vbits |= 1u << (8 * i);
    if (MODE == 1) {
      if (near_in) { off[i][0] = t.yn * W + t.xn; taps |= 1u << (4 * i); }
    } else {
      const bool xa = t.x0 >= 0 && t.x0 < W, xb = t.x0 + 1 >= 0 && t.x0 + 1 < W;
      const bool ya = t.y0 >= 0 && t.y0 < H, yb = t.y0 + 1 >= 0 && t.y0 + 1 < H;
      if (xa && ya) { off[i][0] = t.y0 * W + t.x0; taps |= 1u << (4 * i); }
      if (xb && ya) { off[i][1] = t.y0 * W + t.x0 + 1; taps |= 2u << (4 * i); }
      if (xa && yb) { off[i][2] = (t.y0 + 1) * W + t.x0; taps |= 4u << (4 * i); }
      if (xb && yb) { off[i][3] = (t.y0 + 1) * W + t.x0 + 1; taps |= 8u << (4 * i); }
      wt[i][0] = t.w00; wt[i][1] = t.w01; wt[i][2] = t.w10; wt[i][3] = t.w11;
    }
  }
  const int64_t at = (int64_t)y * W + x;
  if (valid) {
    uint8_t* v = valid + (int64_t)b * plane + at;
    if (vec && n == WARP_PX) *reinterpret_cast<uint32_t*>(v) = vbits;
    else
      for (int i = 0; i < n; ++i) v[i] = (uint8_t)((vbits >> (8 * i)) & 1u);
  }
  for (int c = 0; c < C; ++c) {
    const float* s = src + ((int64_t)b * C + c) * plane;
    float* d = dst + ((int64_t)b * C + c) * plane + at;
    float o[WARP_PX], v[WARP_PX][4];
#pragma unroll
    for (int i = 0; i < WARP_PX; ++i)
#pragma unroll
      for (int k = 0; k < (MODE == 1 ? 1 : 4); ++k) v[i][k] = s[off[i][k]];
#pragma unroll
    for (int i = 0; i < WARP_PX; ++i) {
#pragma unroll
      for (int k = 0; k < (MODE == 1 ? 1 : 4); ++k) v[i][k] = (taps >> (4 * i + k)) & 1u ? v[i][k] : 0.f;
      o[i] = MODE == 1 ? v[i][0] : ((v[i][0] * wt[i][0] + v[i][1] * wt[i][1]) + v[i][2] * wt[i][2]) + v[i][3] * wt[i][3];
    }
    if (vec && n == WARP_PX) *reinterpret_cast<f32x4*>(d) = f32x4{o[0], o[1], o[2], o[3]};
    else
      for (int i = 0; i < n; ++i) d[i] = o[i];
  }
}

constexpr int ERODE_TW = 64, ERODE_TH = 32, ERODE_MAX_R = 8;
constexpr int ERODE_LW = ERODE_TW + 2 * ERODE_MAX_R, ERODE_LH = ERODE_TH + 2 * ERODE_MAX_R;

// grid (ceil(W / ERODE_TW), ceil(H / ERODE_TH), B), block 256
static __global__ __launch_bounds__(256) void erode_kernel(const uint8_t* __restrict__ mask, int H, int W, int r, int vec,
                                                           uint8_t* __restrict__ out) {
  __shared__ __attribute__((aligned(4))) uint8_t tile[ERODE_LH][ERODE_LW];     // tile + halo, 0 / 1
  __shared__ __attribute__((aligned(4))) uint8_t rows[ERODE_LH][ERODE_TW];     // horizontal AND
  const int x0 = blockIdx.x * ERODE_TW, y0 = blockIdx.y * ERODE_TH;
  const int64_t plane = (int64_t)H * W;
  const uint8_t* in = mask + (int64_t)blockIdx.z * plane;
  const int lw = ERODE_TW + 2 * r, lh = ERODE_TH + 2 * r;
  for (int i = threadIdx.x; i < lh * lw; i += 256) {
    const int rr = i / lw, cc = i - rr * lw;
    const int gy = y0 - r + rr, gx = x0 - r + cc;
    const bool inside = gy >= 0 && gy < H && gx >= 0 && gx < W;
    tile[rr][cc] = inside ? (uint8_t)(in[(int64_t)gy * W + gx] != 0) : (uint8_t)1;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < lh * ERODE_TW; i += 256) {
    const int rr = i / ERODE_TW, cc = i % ERODE_TW;
    uint8_t a = 1;
    for (int k = 0; k <= 2 * r; ++k) a &= tile[rr][cc + k];
    rows[rr][cc] = a;
  }
  __syncthreads();
  uint8_t* o = out + (int64_t)blockIdx.z * plane;
  for (int i = threadIdx.x; i < ERODE_TH * (ERODE_TW / 4); i += 256) {
    const int rr = i / (ERODE_TW / 4), c4 = (i % (ERODE_TW / 4)) * 4;
    const int gy = y0 + rr, gx = x0 + c4;
    if (gy >= H || gx >= W) continue;
    uint32_t a = 0x01010101u;
    for (int k = 0; k <= 2 * r; ++k) a &= *reinterpret_cast<const uint32_t*>(&rows[rr + k][c4]);
    uint8_t* p = o + (int64_t)gy * W + gx;
    if (vec && gx + 3 < W) *reinterpret_cast<uint32_t*>(p) = a;
    else
      for (int j = 0; j < 4 && gx + j < W; ++j) p[j] = (uint8_t)((a >> (8 * j)) & 1u);
  }
}

}  // namespace lt
