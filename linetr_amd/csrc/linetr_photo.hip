// liblinetr_hip.so, translation unit 7 of 7: the photometric augmentation of the dataset builder (C ABI in include/linetr_hip.h; kernels
// and the contract of every stage in lt_photometric.h): the host sampler, the workspace layout, the augmentation and the Gaussian blur alone.
#include <algorithm>

#include "lt_handle.h"
#include "lt_photometric.h"

using namespace lt;

namespace {

constexpr int PH_MAX_DIM = 32768, PH_MAX_PLANES = 65535;      // the extents of linetr_warp_images; planes ride on grid.z
constexpr int PH_ALL_STAGES = 127;

int photo_dims_ok(const char* who, int64_t B, int64_t C, int64_t H, int64_t W) {
  if (B < 1 || C < 1 || H < 1 || W < 1) return fail(LINETR_E_ARG, "%s: bad shape B=%lld C=%lld H=%lld W=%lld", who, (long long)B, (long long)C, (long long)H, (long long)W);
  if (B * C > PH_MAX_PLANES || H > PH_MAX_DIM || W > PH_MAX_DIM || H * W * C >= ((int64_t)1 << 31))
    return fail(LINETR_E_ARG, "%s: B * C = %lld above %d, an extent above %d or H * W * C = %lld x %lld x %lld at or beyond 2^31 elements", who,
                (long long)(B * C), PH_MAX_PLANES, PH_MAX_DIM, (long long)H, (long long)W, (long long)C);
  return LINETR_OK;
}

// THE layout of the workspace: the query returns `total`, the calls carve the same segments.
struct PhotoLayout {
  int64_t table, taps, lev, rowsum, lev2, total;
};
PhotoLayout photo_layout(int64_t B, int64_t C, int64_t H, int64_t W) {
  Carve c;
  PhotoLayout l;
  const int64_t plane_bytes = B * C * H * W * (int64_t)sizeof(float);
  l.table = c.take(B * (int64_t)sizeof(LinetrPhotoParams));
  l.taps = c.take(B * 2 * PH_TAPS * (int64_t)sizeof(float));
  l.lev = c.take(plane_bytes);        // the levels after stage 5
  l.rowsum = c.take(plane_bytes);     // the row pass of a blur
  l.lev2 = c.take(plane_bytes);       // the levels after stage 6
  l.total = c.o;
  return l;
}

bool odd_ksize(int k) { return k >= 1 && k <= LINETR_PHOTO_MAX_KSIZE && (k & 1); }

int photo_params_ok(const char* who, const LinetrPhotoParams& p, int b) {
  if (p.stages & ~PH_ALL_STAGES) return fail(LINETR_E_ARG, "%s: image %d has unknown stage bits 0x%x", who, b, p.stages);
  if (p.d < -255 || p.d > 255) return fail(LINETR_E_ARG, "%s: image %d: d = %d outside -255 .. 255", who, b, p.d);
  if (!std::isfinite(p.alpha) || !std::isfinite(p.sigma) || p.sigma < 0 || !std::isfinite(p.blur_sigma) || p.blur_sigma < 0 || !std::isfinite(p.t))
    return fail(LINETR_E_ARG, "%s: image %d: a non-finite parameter or a negative sigma", who, b);
  if (p.K != 1 && p.K != 3 && p.K != 5 && p.K != 7) return fail(LINETR_E_ARG, "%s: image %d: K = %d is none of 1, 3, 5, 7", who, b, p.K);
  for (float w : p.weights)
    if (!std::isfinite(w)) return fail(LINETR_E_ARG, "%s: image %d: a non-finite motion weight", who, b);
  if (!odd_ksize(p.blur_ksize) || !odd_ksize(p.shade_ksize))
    return fail(LINETR_E_ARG, "%s: image %d: ksize %d / %d is even or outside 1 .. %d", who, b, p.blur_ksize, p.shade_ksize, LINETR_PHOTO_MAX_KSIZE);
  if (p.n_ellipses < 0 || p.n_ellipses > LINETR_PHOTO_MAX_ELLIPSES) return fail(LINETR_E_ARG, "%s: image %d: n_ellipses = %d outside 0 .. 20", who, b, p.n_ellipses);
  for (int e = 0; e < p.n_ellipses; ++e) {
    for (double v : p.ellipse[e])
      if (!std::isfinite(v)) return fail(LINETR_E_ARG, "%s: image %d: ellipse %d has a non-finite entry", who, b, e);
    if (!(p.ellipse[e][2] > 0) || !(p.ellipse[e][3] > 0)) return fail(LINETR_E_ARG, "%s: image %d: ellipse %d has an axis <= 0", who, b, e);
  }
  return LINETR_OK;
}

// what both device calls refuse of their tensors and workspace
int photo_buffers_ok(const char* who, const void* d_src, const void* d_dst, const void* ws, int64_t ws_bytes, int64_t need) {
  if (!d_src || !d_dst || !ws) return fail(LINETR_E_ARG, "%s: null pointer", who);
  if (((uintptr_t)d_src | (uintptr_t)d_dst) & 3) return fail(LINETR_E_ARG, "%s: a float tensor that is not 4-byte aligned", who);
  if ((uintptr_t)ws & 255) return fail(LINETR_E_ARG, "%s: a workspace that is not 256-byte aligned", who);
  if (d_src == d_dst) return fail(LINETR_E_ARG, "%s: in-place operation (d_dst == d_src)", who);
  if (ws_bytes < need) return fail(LINETR_E_WORKSPACE, "%s: workspace too small (%lld < %lld bytes)", who, (long long)ws_bytes, (long long)need);
  return LINETR_OK;
}

int photo_carry(const LinetrPhotoParams* params, int B, LinetrPhotoParams* table, float* taps, hipStream_t st) {
  for (int first = 0; first < B; first += PH_CARRY) {
    const int count = std::min(PH_CARRY, B - first);
    PhotoChunk c;
    memset(&c, 0, sizeof c);
    memcpy(c.p, params + first, (size_t)count * sizeof(LinetrPhotoParams));
    hipLaunchKernelGGL(photo_carrier_kernel, dim3((unsigned)count, 2), dim3(64), 0, st, c, first, table, taps);
    LT_LAUNCH_CHECK();
  }
  return LINETR_OK;
}

// one separable blur of [planes][H][W]: src -> rowsum -> dst, epilogue MODE (lt_photometric.h); MASK: the rows come from the ellipses
template <bool MASK, int MODE>
int photo_blur(const float* src, const float* lev, const LinetrPhotoParams* table, const float* taps, int which, int need, int planes, int C,
               int H, int W, int quantise_out, float* rowsum, float* dst, bool any_on, hipStream_t st) {
  if (any_on) {
    hipLaunchKernelGGL(photo_row_kernel<MASK>, dim3((unsigned)cdiv(W, PH_BW), (unsigned)cdiv(H, PH_BR), (unsigned)planes), dim3(256), 0, st, src,
                       table, taps, which, need, C, H, W, rowsum);
    LT_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(photo_col_kernel<MODE>, dim3((unsigned)cdiv(W, PH_CW), (unsigned)cdiv(H, PH_CH), (unsigned)planes), dim3(256), 0, st, rowsum,
                     lev, table, taps, which, need, C, H, W, quantise_out, dst);
  LT_LAUNCH_CHECK();
  return LINETR_OK;
}

double lerp_range(const double (&r)[2], double u) { return r[0] + u * (r[1] - r[0]); }
bool range_ok(const double (&r)[2]) { return std::isfinite(r[0]) && std::isfinite(r[1]) && r[0] <= r[1]; }

}  // namespace

extern "C" int linetr_photometric_sample(const LinetrPhotoConfig* cfg, uint64_t seed, int32_t first, int32_t B, int32_t H, int32_t W,
                                         LinetrPhotoParams* h_params) {
#pragma clang fp contract(off)
  if (!cfg || !h_params) return fail(LINETR_E_ARG, "photometric_sample: null pointer");
  if (B < 1 || H < 1 || W < 1 || first < 0 || (int64_t)first + B > INT32_MAX || seed >> 32)
    return fail(LINETR_E_ARG, "photometric_sample: bad argument (B, H, W >= 1, first >= 0, a 32-bit seed)");
  const LinetrPhotoConfig& c = *cfg;
  if (c.stages & ~PH_ALL_STAGES) return fail(LINETR_E_ARG, "photometric_sample: unknown stage bits 0x%x", c.stages);
  if ((c.stages & LINETR_PHOTO_BRIGHTNESS) && (c.max_abs_change < 0 || c.max_abs_change > 255))
    return fail(LINETR_E_ARG, "photometric_sample: max_abs_change %d outside 0 .. 255", c.max_abs_change);
  if ((c.stages & LINETR_PHOTO_CONTRAST) && !range_ok(c.strength_range)) return fail(LINETR_E_ARG, "photometric_sample: bad strength_range");
  if ((c.stages & LINETR_PHOTO_NOISE) && (!range_ok(c.stddev_range) || c.stddev_range[0] < 0)) return fail(LINETR_E_ARG, "photometric_sample: bad stddev_range");
  if ((c.stages & LINETR_PHOTO_IMPULSE) && (!range_ok(c.prob_range) || c.prob_range[0] < 0 || c.prob_range[1] > 1))
    return fail(LINETR_E_ARG, "photometric_sample: prob_range outside 0 .. 1");
  if ((c.stages & LINETR_PHOTO_MOTION) && (c.max_kernel_size < 3 || c.max_kernel_size > LINETR_PHOTO_MAX_K))
    return fail(LINETR_E_ARG, "photometric_sample: max_kernel_size %d outside 3 .. 7", c.max_kernel_size);
  int blur_ksize = 1;
  if (c.stages & LINETR_PHOTO_BLUR) {
    if (!std::isfinite(c.blur_sigma) || !(c.blur_sigma > 0)) return fail(LINETR_E_ARG, "photometric_sample: blur_sigma must be > 0");
    const double s = c.blur_sigma, k = s < 3.0 ? 2.6 * s : (s < 5.0 ? 3.3 * s : 5.21 * s);
    const double kk = std::max(k, 5.0);
    if (kk > LINETR_PHOTO_MAX_KSIZE - 1) return fail(LINETR_E_ARG, "photometric_sample: blur_sigma %g needs a ksize above %d", s, LINETR_PHOTO_MAX_KSIZE);
    blur_ksize = (int)kk;
    if (blur_ksize % 2 == 0) blur_ksize += 1;
  }
  if (c.stages & LINETR_PHOTO_SHADE) {
    if (c.nb_ellipses < 0 || c.nb_ellipses > LINETR_PHOTO_MAX_ELLIPSES) return fail(LINETR_E_ARG, "photometric_sample: nb_ellipses %d outside 0 .. 20", c.nb_ellipses);
    if (!range_ok(c.transparency_range)) return fail(LINETR_E_ARG, "photometric_sample: bad transparency_range");
    if (c.kernel_size_range[0] < 1 || c.kernel_size_range[1] <= c.kernel_size_range[0] || c.kernel_size_range[1] - 1 > LINETR_PHOTO_MAX_KSIZE)
      return fail(LINETR_E_ARG, "photometric_sample: kernel_size_range [%d, %d) outside 1 .. %d or empty", c.kernel_size_range[0], c.kernel_size_range[1], LINETR_PHOTO_MAX_KSIZE);
    if (c.nb_ellipses > 0 && std::min(H, W) < 20)
      return fail(LINETR_E_ARG, "photometric_sample: min(H, W) = %d below 20: an ellipse axis int(min_dim / 5) would be 0", std::min(H, W));
  }
  for (int b = 0; b < B; ++b) {
    LinetrPhotoParams& p = h_params[b];
    memset(&p, 0, sizeof p);
    const uint32_t image = (uint32_t)(first + b);
    auto draw = [&](uint32_t n, double& u0, double& u1) {
      uint32_t w[4];
      philox4x32_10(n, 0u, 0u, 1u, (uint32_t)seed, image, w);
      u0 = photo_u01(w[0], w[1]);
      u1 = photo_u01(w[2], w[3]);
    };
    double u0, u1;
    p.stages = c.stages & ~LINETR_PHOTO_MOTION;
    p.alpha = 1.0;
    p.K = 1;
    p.weights[0] = 1.f;
    p.blur_ksize = blur_ksize;
    p.blur_sigma = (c.stages & LINETR_PHOTO_BLUR) ? c.blur_sigma : 0.0;
    p.shade_ksize = 1;
    draw(0, u0, u1);
    if (c.stages & LINETR_PHOTO_BRIGHTNESS) p.d = (int)std::floor(u0 * (2.0 * c.max_abs_change + 1.0)) - c.max_abs_change;
    if (c.stages & LINETR_PHOTO_CONTRAST) p.alpha = lerp_range(c.strength_range, u1);
    draw(1, u0, u1);
    if (c.stages & LINETR_PHOTO_NOISE) p.sigma = lerp_range(c.stddev_range, u0);
    if (c.stages & LINETR_PHOTO_IMPULSE) p.thr = (uint32_t)std::min(std::floor(lerp_range(c.prob_range, u1) * 4294967296.0), 4294967295.0);
    draw(2, u0, u1);
    if ((c.stages & LINETR_PHOTO_MOTION) && u0 < 0.5) {
      p.stages |= LINETR_PHOTO_MOTION;
      const int K = 3 + 2 * (int)std::floor(u1 * (double)((c.max_kernel_size - 3) / 2 + 1)), r = K / 2;
      p.K = K;
      draw(3, u0, u1);
      const double theta = M_PI * u0, ct = std::cos(theta), sn = std::sin(theta);
      double w[49], total = 0.0;
      for (int i = 0; i < K; ++i)
        for (int j = 0; j < K; ++j) {
          const double a = ct * (double)(i - r), bb = sn * (double)(j - r);
          w[i * K + j] = std::max(0.0, 1.0 - std::fabs(a - bb));
          total += w[i * K + j];
        }
      for (int i = 0; i < K * K; ++i) p.weights[i] = (float)(w[i] / total);
    }
    if (c.stages & LINETR_PHOTO_SHADE) {
      draw(4, u0, u1);
      p.t = lerp_range(c.transparency_range, u0);
      int ks = c.kernel_size_range[0] + (int)std::floor(u1 * (double)(c.kernel_size_range[1] - c.kernel_size_range[0]));
      if (ks % 2 == 0) ks += 1;
      p.shade_ksize = ks;
      p.n_ellipses = c.nb_ellipses;
      const double min_dim = (double)std::min(H, W) / 4.0;
      for (int e = 0; e < c.nb_ellipses; ++e) {
        draw(5 + 3 * (uint32_t)e, u0, u1);
        const int ax = (int)std::max(u0 * min_dim, min_dim / 5.0), ay = (int)std::max(u1 * min_dim, min_dim / 5.0);
        const int max_rad = std::max(ax, ay);
        draw(6 + 3 * (uint32_t)e, u0, u1);
        const int cx = max_rad + (int)std::floor(u0 * (double)(W - 2 * max_rad)), cy = max_rad + (int)std::floor(u1 * (double)(H - 2 * max_rad));
        draw(7 + 3 * (uint32_t)e, u0, u1);
        const double ang = (u0 * 90.0) * (M_PI / 180.0);
        double* q = p.ellipse[e];
        q[0] = cx; q[1] = cy; q[2] = ax; q[3] = ay; q[4] = std::cos(ang); q[5] = std::sin(ang);
      }
    }
  }
  return LINETR_OK;
}

extern "C" int64_t linetr_photometric_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W) {
  if (photo_dims_ok("photometric_workspace_bytes", B, C, H, W)) return 0;
  return photo_layout(B, C, H, W).total;
}

extern "C" int linetr_photometric_tile(int32_t* tile_h, int32_t* tile_w, int32_t* halo, int32_t* row_tile_h, int32_t* row_tile_w,
                                       int32_t* col_tile_h, int32_t* col_tile_w, int32_t* max_radius) {
  if (!tile_h || !tile_w || !halo || !row_tile_h || !row_tile_w || !col_tile_h || !col_tile_w || !max_radius)
    return fail(LINETR_E_ARG, "photometric_tile: null pointer");
  *tile_h = PH_TH; *tile_w = PH_TW; *halo = PH_HALO;
  *row_tile_h = PH_BR; *row_tile_w = PH_BW;
  *col_tile_h = PH_CH; *col_tile_w = PH_CW;
  *max_radius = PH_MAX_R;
  return LINETR_OK;
}

extern "C" int linetr_photometric(LinetrHandle* h, const float* d_src, int32_t B, int32_t H, int32_t W, const LinetrPhotoParams* h_params,
                                  uint64_t seed, int32_t first, int32_t quantise_out, float* d_dst, void* d_workspace, int64_t workspace_bytes,
                                  void* stream) {
  // every refusal comes before the first launch
  if (int e = photo_dims_ok("photometric", B, 1, H, W)) return e;
  if (!h_params) return fail(LINETR_E_ARG, "photometric: null pointer");
  if (seed >> 32 || first < 0 || (int64_t)first + B > INT32_MAX) return fail(LINETR_E_ARG, "photometric: a seed beyond 32 bits or a bad first image");
  if (quantise_out != 0 && quantise_out != 1) return fail(LINETR_E_ARG, "photometric: quantise_out %d is neither 0 nor 1", quantise_out);
  int any = 0;
  for (int b = 0; b < B; ++b) {
    if (int e = photo_params_ok("photometric", h_params[b], b)) return e;
    any |= h_params[b].stages;
  }
  const PhotoLayout l = photo_layout(B, 1, H, W);
  if (int e = photo_buffers_ok("photometric", d_src, d_dst, d_workspace, workspace_bytes, l.total)) return e;
  if (h) LT_HIP(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  char* ws = static_cast<char*>(d_workspace);
  LinetrPhotoParams* table = reinterpret_cast<LinetrPhotoParams*>(ws + l.table);
  float* taps = reinterpret_cast<float*>(ws + l.taps);
  float *lev = reinterpret_cast<float*>(ws + l.lev), *rowsum = reinterpret_cast<float*>(ws + l.rowsum), *lev2 = reinterpret_cast<float*>(ws + l.lev2);
  const double px = (double)B * H * W;
  ProfScope ps(h, st, "photometric", 0, px * 24.0);
  if (int e = photo_carry(h_params, B, table, taps, st)) return e;
  const int vec = W % 4 == 0 && aligned16(d_src);
  hipLaunchKernelGGL(photo_point_kernel, dim3((unsigned)cdiv(W, PH_TW), (unsigned)cdiv(H, PH_TH), (unsigned)B), dim3(256), 0, st, d_src, table,
                     (uint32_t)seed, first, H, W, vec, lev);
  LT_LAUNCH_CHECK();
  const float* cur = lev;
  if (any & LINETR_PHOTO_BLUR) {
    if (int e = photo_blur<false, 1>(lev, lev, table, taps, 0, LINETR_PHOTO_BLUR, B, 1, H, W, 0, rowsum, lev2, true, st)) return e;
    cur = lev2;
  }
  return photo_blur<true, 2>(nullptr, cur, table, taps, 1, LINETR_PHOTO_SHADE, B, 1, H, W, quantise_out, rowsum, d_dst, any & LINETR_PHOTO_SHADE, st);
}

extern "C" int linetr_gaussian_blur(LinetrHandle* h, const float* d_src, int32_t B, int32_t C, int32_t H, int32_t W, const int32_t* h_ksize,
                                    const double* h_sigma, int32_t quantise, float* d_dst, void* d_workspace, int64_t workspace_bytes,
                                    void* stream) {
  if (int e = photo_dims_ok("gaussian_blur", B, C, H, W)) return e;
  if (!h_ksize || !h_sigma) return fail(LINETR_E_ARG, "gaussian_blur: null pointer");
  if (quantise != 0 && quantise != 1) return fail(LINETR_E_ARG, "gaussian_blur: quantise %d is neither 0 nor 1", quantise);
  for (int b = 0; b < B; ++b)
    if (!odd_ksize(h_ksize[b]) || !std::isfinite(h_sigma[b]) || h_sigma[b] < 0)
      return fail(LINETR_E_ARG, "gaussian_blur: image %d: ksize %d even or outside 1 .. %d, or a sigma that is negative or not finite", b, h_ksize[b], LINETR_PHOTO_MAX_KSIZE);
  const PhotoLayout l = photo_layout(B, C, H, W);
  if (int e = photo_buffers_ok("gaussian_blur", d_src, d_dst, d_workspace, workspace_bytes, l.total)) return e;
  if (h) LT_HIP(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  char* ws = static_cast<char*>(d_workspace);
  LinetrPhotoParams* table = reinterpret_cast<LinetrPhotoParams*>(ws + l.table);
  float* taps = reinterpret_cast<float*>(ws + l.taps);
  float* rowsum = reinterpret_cast<float*>(ws + l.rowsum);
  ProfScope ps(h, st, "gaussian_blur", 0, (double)B * C * H * W * 16.0);
  for (int first = 0; first < B; first += PH_CARRY) {
    const int count = std::min(PH_CARRY, B - first);
    LinetrPhotoParams p[PH_CARRY];
    memset(p, 0, sizeof p);
    for (int i = 0; i < count; ++i) {
      p[i].stages = LINETR_PHOTO_BLUR;
      p[i].K = 1;
      p[i].blur_ksize = h_ksize[first + i];
      p[i].blur_sigma = h_sigma[first + i];
      p[i].shade_ksize = 1;
    }
    if (int e = photo_carry(p, count, table + first, taps + (int64_t)first * 2 * PH_TAPS, st)) return e;
  }
  if (quantise) return photo_blur<false, 1>(d_src, d_src, table, taps, 0, LINETR_PHOTO_BLUR, B * C, C, H, W, 0, rowsum, d_dst, true, st);
  return photo_blur<false, 0>(d_src, d_src, table, taps, 0, LINETR_PHOTO_BLUR, B * C, C, H, W, 0, rowsum, d_dst, true, st);
}
