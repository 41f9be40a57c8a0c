// Ground-truth line assignment of a homography pair on the device: what the reference's dataset builder computes per pair
// (dataloaders/build_homography_dataset.py:210-237) with two Python double loops (dataloaders/utils/util_lines.py:67-171):
//   klns0_projected = perspectiveTransform(klns0, H), klns1_projected = perspectiveTransform(klns1, inv(H))          :214-218
//   find_line_matches both ways, calculate_line_overlaps both ways                                                    :222-232
//   mat_assign_sublines = the larger overlap where both directions matched; lmatches = where(. > min_overlap_ratio)   :225-234
// Three launches for a batch of B pairs with n0 / n1 sub-lines per side:
//   gt_lines_kernel   grid (lines / 256, B): every line ONCE -- its projection (double arithmetic, cast to the coordinate type) and the
//                     angle degrees(arctan2(dx, dy)) of the line and of its projection (four angle arrays per item, not per pair);
//   gt_pair_kernel    grid (column tiles of 64, row groups of GT_ROWS, B): one thread per (i, j), the column's two lines in registers,
//                     the row's two lines wave-uniform.  Both directions of the match test and of calc_overlap, the assignment
//                     (with its zero dustbin row and column), the per-direction matrices, and per row and 64 columns one ballot
//                     word of `assign > min_overlap_ratio`;
//   gt_list_kernel    grid (B): popcounts of the rows' words, a block scan, then every row emits its pairs in column order -- the
//                     row-major order of np.where, no atomics; -1 behind the list; found is not capped, nothing is written past M.
// Arithmetic: templated on the coordinate type T.  float is the reference as executed (its sub-lines are float32 tensors, so NumPy
// computes every scalar in float32), double is for float64 geometry.  No contraction, the reference's operation order, x * x for
// ** 2, IEEE divide and square root (the build has no fast-math flag; HIP's default keeps float divide and sqrt correctly rounded):
// every compare except the angle one is the reference's bit for bit.  atan2 is the one operation that is not correctly rounded on
// both sides: an entry can differ from the reference's only where |angle difference % 180 - thres_angdiff| (or the distance of the
// difference from the wrap at 180 / 360) is within a few ulp of the angles.
#pragma once
#include "lt_parts.h"

namespace lt {

constexpr int GT_ROWS = 16;   // rows of a gt_pair_kernel block: four per wave

template <typename T> struct GtLine { T sx, sy, ex, ey; };

template <typename T> __device__ __forceinline__ T gt_sqrt(T x);
template <> __device__ __forceinline__ float gt_sqrt<float>(float x) { return __builtin_sqrtf(x); }
template <> __device__ __forceinline__ double gt_sqrt<double>(double x) { return __builtin_sqrt(x); }
template <typename T> __device__ __forceinline__ T gt_abs(T x) { return __builtin_fabs(x); }
template <> __device__ __forceinline__ float gt_abs<float>(float x) { return __builtin_fabsf(x); }
// the largest of a list as np.max gives it: a NaN stays
template <typename T> __device__ __forceinline__ T gt_max(T a, T b) { return (a > b || a != a) ? a : b; }
__device__ __forceinline__ float gt_atan2(float y, float x) { return atan2f(y, x); }
__device__ __forceinline__ double gt_atan2(double y, double x) { return atan2(y, x); }
__device__ __forceinline__ float gt_fmod(float a, float b) { return fmodf(a, b); }
__device__ __forceinline__ double gt_fmod(double a, double b) { return fmod(a, b); }

// cv2.perspectiveTransform's arithmetic for one point: double accumulation, the result cast to the coordinate type
template <typename T>
__device__ __forceinline__ void gt_project(const double* __restrict__ m, T x_, T y_, T& X, T& Y) {
#pragma clang fp contract(off)
  const double x = (double)x_, y = (double)y_;
  double w = x * m[6] + y * m[7] + m[8];
  w = (w != 0.0) ? 1.0 / w : 0.0;
  X = (T)((x * m[0] + y * m[1] + m[2]) * w);
  Y = (T)((x * m[3] + y * m[4] + m[5]) * w);
}

// util_lines.py:84-85: np.degrees(np.arctan2(dx, dy)); NumPy's degrees multiplies by the constant 180 / pi evaluated in T
template <typename T>
__device__ __forceinline__ T gt_angle(const GtLine<T>& l) {
#pragma clang fp contract(off)
  constexpr T RAD2DEG = (T)180 / (T)3.141592653589793238462643383279502884;
  return gt_atan2(l.ex - l.sx, l.ey - l.sy) * RAD2DEG;
}

// lines [B][n][2][2] -> proj [B][n][2][2] (through m = H [item][which]), ang / ang_proj [B][n].  grid (cdiv(n, 256), B)
template <typename T>
__global__ __launch_bounds__(256) void gt_lines_kernel(const T* __restrict__ lines, int n, const double* __restrict__ H, int which,
                                                       T* __restrict__ proj, T* __restrict__ ang, T* __restrict__ ang_proj) {
  const int item = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double* m = H + ((int64_t)item * 2 + which) * 9;
  const int64_t o = (int64_t)item * n + i;
  const GtLine<T> l = reinterpret_cast<const GtLine<T>*>(lines)[o];
  GtLine<T> p;
  gt_project(m, l.sx, l.sy, p.sx, p.sy);
  gt_project(m, l.ex, l.ey, p.ex, p.ey);
  reinterpret_cast<GtLine<T>*>(proj)[o] = p;
  ang[o] = gt_angle(l);
  ang_proj[o] = gt_angle(p);
}

// calc_distance_point_line (util_lines.py:5-13) and calc_distance_point_point (:15-21)
template <typename T>
__device__ __forceinline__ T gt_point_line(T x0, T y0, const GtLine<T>& l) {
#pragma clang fp contract(off)
  const T a = l.ey - l.sy, b = l.ex - l.sx;
  return gt_abs(a * x0 - b * y0 + l.ex * l.sy - l.ey * l.sx) / gt_sqrt(a * a + b * b);
}
template <typename T>
__device__ __forceinline__ T gt_point_point(T x0, T y0, T x1, T y1) {
#pragma clang fp contract(off)
  const T dx = x1 - x0, dy = y1 - y0;
  return gt_sqrt(dx * dx + dy * dy);
}

// One direction for one pair: `ref` is the reference line (line0 of util_lines.py), `oth` the other image's line projected into its
// frame.  find_line_matches (:67-114) -> match; calc_overlap (:117-154) -> the return value, evaluated whether or not it matched.
// Every compare is written as the reference writes it, so a NaN (a zero-length reference line: 0 / 0) falls where it falls there.
template <typename T>
__device__ __forceinline__ T gt_direction(const GtLine<T>& ref, T ang_ref, const GtLine<T>& oth, T ang_oth, T thres_reprojected,
                                          T thres_angdiff, bool& match) {
#pragma clang fp contract(off)
  const T dist0 = gt_point_line(oth.sx, oth.sy, ref);
  const T dist1 = gt_point_line(oth.ex, oth.ey, ref);
  const bool too_far = dist0 > thres_reprojected && dist1 > thres_reprojected;         // :80 (an `and`)
  const T ang_diff = gt_fmod(gt_abs(ang_oth - ang_ref), (T)180);                        // :87-88 (both operands >= 0: % is fmod)
  const bool turned = ang_diff > thres_angdiff;                                         // :90
  const T len0 = gt_point_point(ref.sx, ref.sy, ref.ex, ref.ey);
  const T len1 = gt_point_point(oth.sx, oth.sy, oth.ex, oth.ey);
  const T s0s1 = gt_point_point(ref.sx, ref.sy, oth.sx, oth.sy);
  const T e0s1 = gt_point_point(ref.ex, ref.ey, oth.sx, oth.sy);
  const T s0e1 = gt_point_point(ref.sx, ref.sy, oth.ex, oth.ey);
  const T e0e1 = gt_point_point(ref.ex, ref.ey, oth.ex, oth.ey);
  const bool sp_on = s0s1 < len0 && e0s1 < len0;
  const bool ep_on = s0e1 < len0 && e0e1 < len0;
  const T dmax = gt_max(gt_max(s0s1, e0s1), gt_max(s0e1, e0e1));
  const T lsum = len0 + len1;
  const bool apart = !sp_on && !ep_on && dmax > lsum;                                   // :105-108
  match = !too_far && !turned && !apart;
  if (sp_on && ep_on) return len1 / len0;
  if (sp_on) return (s0e1 > e0e1 ? e0s1 : s0s1) / len0;
  if (ep_on) return (s0s1 > e0s1 ? e0e1 : s0e1) / len0;
  return dmax <= lsum ? (T)1 : (T)0;
}

// grid (cdiv(n1 + pad, 64), cdiv(n0 + pad, GT_ROWS), B), block 256.  lines / proj [B][n][2][2], the four angle arrays [B][n].
// Outputs (any may be null): assign [B][n0 + pad][n1 + pad] float32; match_dir [B][2][n0][n1] uint8 and overlap_dir [B][2][n0][n1] T,
// direction 1 stored as [i][j]; words [B][n0][cdiv(n1, 64)]: bit j % 64 of word j / 64 of row i = assign[i][j] > min_overlap.
template <typename T>
__global__ __launch_bounds__(256) void gt_pair_kernel(const T* __restrict__ lines0, const T* __restrict__ lines1,
                                                      const T* __restrict__ proj0, const T* __restrict__ proj1,
                                                      const T* __restrict__ ang0, const T* __restrict__ ang1,
                                                      const T* __restrict__ angp0, const T* __restrict__ angp1, int n0, int n1,
                                                      const int* __restrict__ count0, const int* __restrict__ count1,
                                                      T thres_reprojected, T thres_angdiff, double min_overlap, int pad,
                                                      float* __restrict__ assign, unsigned char* __restrict__ match_dir,
                                                      T* __restrict__ overlap_dir, unsigned long long* __restrict__ words) {
  const int item = blockIdx.z, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = blockIdx.x * 64 + lane;
  const int c0 = count0 ? min(max(count0[item], 0), n0) : n0;
  const int c1 = count1 ? min(max(count1[item], 0), n1) : n1;
  const int ld = n1 + pad, W64 = (n1 + 63) >> 6;
  const bool col_ok = j < c1;
  const int jc = min(j, n1 - 1);
  const GtLine<T> l1 = reinterpret_cast<const GtLine<T>*>(lines1)[(int64_t)item * n1 + jc];
  const GtLine<T> p1 = reinterpret_cast<const GtLine<T>*>(proj1)[(int64_t)item * n1 + jc];
  const T a1 = ang1[(int64_t)item * n1 + jc], ap1 = angp1[(int64_t)item * n1 + jc];
#pragma unroll 1
  for (int r = 0; r < GT_ROWS / 4; ++r) {
    const int i = __builtin_amdgcn_readfirstlane(blockIdx.y * GT_ROWS + wave * (GT_ROWS / 4) + r);
    if (i >= n0 + pad) break;
    T value = (T)0, ov0 = (T)0, ov1 = (T)0;
    bool m0 = false, m1 = false;
    if (i < c0 && col_ok) {
      const GtLine<T> l0 = reinterpret_cast<const GtLine<T>*>(lines0)[(int64_t)item * n0 + i];
      const GtLine<T> p0 = reinterpret_cast<const GtLine<T>*>(proj0)[(int64_t)item * n0 + i];
      const T a0 = ang0[(int64_t)item * n0 + i], ap0 = angp0[(int64_t)item * n0 + i];
      ov0 = gt_direction(l0, a0, p1, ap1, thres_reprojected, thres_angdiff, m0);      // lines0[i] against proj(lines1[j], Hinv)
      ov1 = gt_direction(l1, a1, p0, ap0, thres_reprojected, thres_angdiff, m1);      // lines1[j] against proj(lines0[i], H)
      if (m0 && m1) value = ov0 > ov1 ? ov0 : ov1;                                    // :233
    }
    if (assign && j < ld) assign[((int64_t)item * (n0 + pad) + i) * ld + j] = (float)value;
    if (i < n0) {
      // (the reference's matrix is float64 and holds the value exactly: the compare is made there, not on the rounded float32)
      const unsigned long long word = __ballot(i < c0 && col_ok && (double)value > min_overlap);
      if (words && lane == 0 && (int)blockIdx.x < W64) words[((int64_t)item * n0 + i) * W64 + blockIdx.x] = word;
      if (j < n1) {
        const int64_t o = ((int64_t)item * 2 * n0 + i) * n1 + j, o1 = o + (int64_t)n0 * n1;
        if (match_dir) { match_dir[o] = m0; match_dir[o1] = m1; }
        if (overlap_dir) { overlap_dir[o] = ov0; overlap_dir[o1] = ov1; }
      }
    }
  }
}

// grid (B), block 256.  lmatches [B][M][2] (may be null), found [B].
__global__ __launch_bounds__(256) void gt_list_kernel(const unsigned long long* __restrict__ words, int n0, int W64, int M,
                                                      int* __restrict__ lmatches, int* __restrict__ found) {
  __shared__ int part[256];
  const int item = blockIdx.x, t = threadIdx.x;
  int* lm = lmatches ? lmatches + (int64_t)item * M * 2 : nullptr;
  int carry = 0;
  for (int base = 0; base < n0; base += 256) {
    const int i = base + t;
    const unsigned long long* row = words + ((int64_t)item * n0 + min(i, n0 - 1)) * W64;
    int c = 0;
    if (i < n0)
      for (int w = 0; w < W64; ++w) c += __popcll(row[w]);
    int sum;
    int rank = carry + kp_block_scan(c, part, sum);
    if (lm && i < n0) {
      for (int w = 0; w < W64 && rank < M; ++w) {
        unsigned long long m = row[w];
        while (m && rank < M) {
          lm[2 * rank] = i;
          lm[2 * rank + 1] = w * 64 + __ffsll(m) - 1;
          m &= m - 1;
          ++rank;
        }
      }
    }
    carry += sum;
  }
  if (lm)
    for (int r = min(carry, M) + t; r < M; r += 256) { lm[2 * r] = -1; lm[2 * r + 1] = -1; }
  if (t == 0) found[item] = carry;
}

}  // namespace lt
