// liblinetr_hip.so, translation unit 6 of 6: the line segment detector (C ABI in include/linetr_hip.h; kernels in lt_linedet.h).
// linetr_detect_lines and the two entry points that run a part of it alone for the unit tests.  No LinetrHandle state: `h` only
// carries the profiler.
#include <algorithm>

#include "lt_handle.h"
#include "lt_linedet.h"

using namespace lt;

namespace {

constexpr int DET_MAX_B = 32767;      // both partitions of a batch share grid.y / grid.z

struct DetLayout {
  int64_t off[DET_MAX_OCT][12];
  int64_t o_counts, total;
  DetOct oct[DET_MAX_OCT];            // extents only
};

// Octave extents and the offset of every array.  B, H, W, n_oct have been validated.
DetLayout det_layout(int B, int H, int W, int n_oct) {
  DetLayout L{};
  Carve c;
  int h = H, w = W;
  for (int i = 0; i < n_oct; ++i) {
    DetOct& o = L.oct[i];
    o.H = h; o.W = w;
    o.Hc = (h >= 2 && w >= 2) ? h - 1 : 0;
    o.Wc = (h >= 2 && w >= 2) ? w - 1 : 0;
    const int64_t nc = (int64_t)o.Hc * o.Wc, np = (int64_t)h * w;
    o.cap = (int)(nc / DET_MIN_REGION) + 1;
    int64_t* f = L.off[i];
    f[0] = c.take(B * np);
    f[1] = c.take(B * nc * 4);
    f[2] = c.take(2 * B * nc);
    f[3] = c.take(2 * B * nc * 4);
    f[4] = c.take(2 * B * nc * 4);
    f[5] = c.take(2 * B * nc * 4);
    f[6] = c.take(2 * B * nc * 4);
    f[7] = c.take(2LL * B * o.cap * 4);
    f[8] = c.take(2LL * B * o.cap * 7 * 8);
    f[9] = c.take(2LL * B * o.cap * 4 * 8);
    f[10] = c.take(2LL * B * o.cap * 4 * 8);
    f[11] = c.take(2LL * B * 4);
    h = (h + 1) / 2;
    w = (w + 1) / 2;
  }
  L.o_counts = c.take((int64_t)B * n_oct * 4);
  L.total = c.o;
  return L;
}

void det_bind(DetLayout& L, int n_oct, void* ws) {
  char* p = (char*)ws;
  for (int i = 0; i < n_oct; ++i) {
    DetOct& o = L.oct[i];
    const int64_t* f = L.off[i];
    o.q = (uint8_t*)(p + f[0]);
    o.m2 = (int32_t*)(p + f[1]);
    o.bk = (int8_t*)(p + f[2]);
    o.raw = (int32_t*)(p + f[3]);
    o.lab = (int32_t*)(p + f[4]);
    o.size = (int32_t*)(p + f[5]);
    o.votes = (int32_t*)(p + f[6]);
    o.c_label = (int32_t*)(p + f[7]);
    o.c_acc = (long long*)(p + f[8]);
    o.c_geo = (double*)(p + f[9]);
    o.c_ext = (long long*)(p + f[10]);
    o.c_count = (int32_t*)(p + f[11]);
  }
}

int det_dims_ok(const char* who, int B, int H, int W) {
  if (B < 1 || B > DET_MAX_B) return fail(LINETR_E_ARG, "%s: B=%d outside 1..%d", who, B, DET_MAX_B);
  if (H < 1 || W < 1 || H > DET_MAX_DIM || W > DET_MAX_DIM) return fail(LINETR_E_ARG, "%s: H=%d W=%d outside 1..%d", who, H, W, DET_MAX_DIM);
  return LINETR_OK;
}

int det_config_ok(const char* who, const LinetrDetectConfig* cfg) {
  if (!cfg) return fail(LINETR_E_ARG, "%s: null config", who);
  if (cfg->n_octaves < 1 || cfg->n_octaves > DET_MAX_OCT) return fail(LINETR_E_ARG, "%s: n_octaves %d outside 1..%d", who, cfg->n_octaves, DET_MAX_OCT);
  if (cfg->scale != 2) return fail(LINETR_E_ARG, "%s: scale %d: only 2 is supported", who, cfg->scale);
  if (cfg->grad_threshold < 1) return fail(LINETR_E_ARG, "%s: grad_threshold %d below 1", who, cfg->grad_threshold);
  if (cfg->min_region_size < DET_MIN_REGION) return fail(LINETR_E_ARG, "%s: min_region_size %d below %d", who, cfg->min_region_size, DET_MIN_REGION);
  if (!(cfg->density >= 0.0 && cfg->density <= 1.0)) return fail(LINETR_E_ARG, "%s: density outside 0..1", who);
  return LINETR_OK;
}

// quantise + pyramid: octave 0 .. n_oct - 1 of the batch.  Returns where octave 0 lives (a uint8 input is used in place).
int det_pyramid(LinetrHandle* h, const void* d_images, int is_float, int B, DetLayout& L, int n_oct, hipStream_t st) {
  DetOct& o0 = L.oct[0];
  const int64_t n0 = (int64_t)B * o0.H * o0.W;
  if (is_float) {
    ProfScope ps(h, st, "det_quantise", 0, 5.0 * n0);
    hipLaunchKernelGGL(det_quantise_kernel, dim3((unsigned)((n0 + 255) / 256)), dim3(256), 0, st, (const float*)d_images, n0, o0.q);
    LT_LAUNCH_CHECK();
  } else {
    o0.q = (uint8_t*)const_cast<void*>(d_images);
  }
  for (int i = 1; i < n_oct; ++i) {
    const DetOct &a = L.oct[i - 1], &b = L.oct[i];
    ProfScope ps(h, st, "det_pyramid", 0, (double)B * ((double)a.H * a.W + (double)b.H * b.W));
    hipLaunchKernelGGL(det_pyramid_kernel, dim3((unsigned)cdiv(b.W, 64), (unsigned)cdiv(b.H, 4), (unsigned)B), dim3(256), 0, st, a.q, a.H, a.W, b.q,
                       b.H, b.W);
    LT_LAUNCH_CHECK();
  }
  return LINETR_OK;
}

int det_gradient(LinetrHandle* h, const DetOct& o, int B, int thr, int32_t* m2, int8_t* bkA, int8_t* bkB, hipStream_t st) {
  const double nc = (double)B * o.Hc * o.Wc;
  ProfScope ps(h, st, "det_gradient", 0, (double)B * o.H * o.W + 6.0 * nc);
  hipLaunchKernelGGL(det_gradient_kernel, dim3((unsigned)cdiv(o.Wc, DET_T), (unsigned)cdiv(o.Hc, DET_T), (unsigned)B), dim3(256), 0, st, o.q, o.H,
                     o.W, thr, m2, bkA, bkB);
  LT_LAUNCH_CHECK();
  return LINETR_OK;
}

// labels of `images` bucket maps of Hc x Wc cells: raw holds the parent links, lab the result; size / votes (or NULL) are zeroed
int det_label(LinetrHandle* h, const int8_t* bk, int images, int Hc, int Wc, int32_t* raw, int32_t* lab, int32_t* size, int32_t* votes,
              hipStream_t st) {
  const dim3 tiles((unsigned)cdiv(Wc, DET_T), (unsigned)cdiv(Hc, DET_T), (unsigned)images);
  const int Nc = Hc * Wc;
  const double cells = (double)images * Nc;
  {
    ProfScope ps(h, st, "det_label_tile", 0, 5.0 * cells);
    hipLaunchKernelGGL(det_label_tile_kernel, tiles, dim3(256), 0, st, bk, Hc, Wc, raw);
    LT_LAUNCH_CHECK();
  }
  {
    ProfScope ps(h, st, "det_label_merge", 0, cells * 3.0 * 5.0 / DET_T);
    hipLaunchKernelGGL(det_label_merge_kernel, tiles, dim3(3 * DET_T), 0, st, bk, Hc, Wc, raw);
    LT_LAUNCH_CHECK();
  }
  {
    ProfScope ps(h, st, "det_label_flatten", 0, (size ? 20.0 : 12.0) * cells);
    hipLaunchKernelGGL(det_label_flatten_kernel, dim3((unsigned)cdiv(Nc, 256), (unsigned)images), dim3(256), 0, st, raw, Nc, lab, size, votes);
    LT_LAUNCH_CHECK();
  }
  return LINETR_OK;
}

}  // namespace

extern "C" int linetr_detect_tile(int32_t* tile_h, int32_t* tile_w) {
  if (!tile_h || !tile_w) return fail(LINETR_E_ARG, "detect_tile: null pointer");
  *tile_h = DET_T;
  *tile_w = DET_T;
  return LINETR_OK;
}

extern "C" int64_t linetr_detect_lines_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t n_octaves) {
  if (B < 1 || B > DET_MAX_B || H < 1 || W < 1 || H > DET_MAX_DIM || W > DET_MAX_DIM || n_octaves < 1 || n_octaves > DET_MAX_OCT) return 0;
  return det_layout(B, H, W, n_octaves).total;
}

extern "C" int linetr_detect_lines(LinetrHandle* h, const void* d_images, int32_t images_are_float, int32_t B, int32_t H, int32_t W,
                                   const LinetrDetectConfig* cfg, int32_t capacity, double* d_rows, int32_t* h_counts, int64_t* d_debug_regions,
                                   void* d_workspace, int64_t workspace_bytes, void* stream) {
  // every refusal comes before the first launch
  if (int e = det_dims_ok("detect_lines", B, H, W)) return e;
  if (int e = det_config_ok("detect_lines", cfg)) return e;
  if (!d_images || !d_rows || !h_counts || !d_workspace) return fail(LINETR_E_ARG, "detect_lines: null pointer");
  if (images_are_float != 0 && images_are_float != 1) return fail(LINETR_E_ARG, "detect_lines: images_are_float %d is neither 0 nor 1", images_are_float);
  if (capacity < 0) return fail(LINETR_E_ARG, "detect_lines: capacity %d below 0", capacity);
  if ((images_are_float && ((uintptr_t)d_images & 3)) || ((uintptr_t)d_rows & 7) || ((uintptr_t)d_debug_regions & 7) || ((uintptr_t)h_counts & 3) ||
      ((uintptr_t)d_workspace & 255))
    return fail(LINETR_E_ARG, "detect_lines: misaligned rows (float32 images 4, rows and debug rows 8, counts 4, workspace 256 bytes)");
  const int n_oct = cfg->n_octaves;
  DetLayout L = det_layout(B, H, W, n_oct);
  if (workspace_bytes < L.total) return fail(LINETR_E_ARG, "detect_lines: workspace too small (need %lld)", (long long)L.total);
  det_bind(L, n_oct, d_workspace);
  if (h) LT_HIP(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  if (int e = det_pyramid(h, d_images, images_are_float, B, L, n_oct, st)) return e;
  for (int i = 0; i < n_oct; ++i) {
    const DetOct& o = L.oct[i];
    if (o.Hc == 0) continue;
    const int Nc = o.Hc * o.Wc;
    const int64_t part = (int64_t)B * Nc;
    const double cells = (double)B * Nc;
    if (int e = det_gradient(h, o, B, cfg->grad_threshold, o.m2, o.bk, o.bk + part, st)) return e;
    if (int e = det_label(h, o.bk, 2 * B, o.Hc, o.Wc, o.raw, o.lab, o.size, o.votes, st)) return e;
    const dim3 per_cell((unsigned)cdiv(Nc, 256), (unsigned)(2 * B));
    {
      ProfScope ps(h, st, "det_size", 0, 2.0 * cells * 4);
      hipLaunchKernelGGL(det_size_kernel, per_cell, dim3(256), 0, st, o.lab, Nc, o.size);
      LT_LAUNCH_CHECK();
    }
    {
      ProfScope ps(h, st, "det_vote", 0, 2.0 * cells * 8);
      hipLaunchKernelGGL(det_vote_kernel, dim3((unsigned)cdiv(Nc, 256), (unsigned)B), dim3(256), 0, st, o.lab, o.size, Nc, B, o.votes);
      LT_LAUNCH_CHECK();
    }
    {
      ProfScope ps(h, st, "det_assign", 0, 2.0 * cells * 12);
      hipLaunchKernelGGL(det_assign_kernel, dim3((unsigned)(2 * B)), dim3(1024), 0, st, o, cfg->min_region_size);
      LT_LAUNCH_CHECK();
    }
    {
      ProfScope ps(h, st, "det_moments", 0, 2.0 * cells * 8 + cells * 4);
      hipLaunchKernelGGL(det_moment_kernel, per_cell, dim3(256), 0, st, o, B);
      LT_LAUNCH_CHECK();
    }
    {
      ProfScope ps(h, st, "det_fit", 0, 0);
      hipLaunchKernelGGL(det_fit_kernel, dim3((unsigned)cdiv(o.cap, 256), (unsigned)(2 * B)), dim3(256), 0, st, o);
      LT_LAUNCH_CHECK();
    }
    {
      ProfScope ps(h, st, "det_extent", 0, 2.0 * cells * 8);
      hipLaunchKernelGGL(det_extent_kernel, per_cell, dim3(256), 0, st, o);
      LT_LAUNCH_CHECK();
    }
  }
  DetPlan plan{};
  for (int i = 0; i < n_oct; ++i) plan.o[i] = L.oct[i];
  int32_t* d_counts = (int32_t*)((char*)d_workspace + L.o_counts);
  {
    ProfScope ps(h, st, "det_keep", 0, 0);
    hipLaunchKernelGGL(det_keep_kernel, dim3((unsigned)B), dim3(256), 0, st, plan, n_oct, B, cfg->density, capacity, d_rows, d_counts,
                       (long long*)d_debug_regions);
    LT_LAUNCH_CHECK();
  }
  LT_HIP(hipMemcpyAsync(h_counts, d_counts, (size_t)B * n_oct * 4, hipMemcpyDeviceToHost, st));
  return LINETR_OK;
}

extern "C" int64_t linetr_detect_debug_labels_workspace_bytes(int32_t B, int32_t H, int32_t W) {
  if (B < 1 || B > 2 * DET_MAX_B || H < 1 || W < 1 || H > DET_MAX_DIM || W > DET_MAX_DIM) return 0;
  return align_up((int64_t)B * H * W * 4, 256);
}

extern "C" int linetr_detect_debug_labels(LinetrHandle* h, const int8_t* d_buckets, int32_t B, int32_t H, int32_t W, int32_t* d_labels,
                                          void* d_workspace, int64_t workspace_bytes, void* stream) {
  if (B < 1 || B > 2 * DET_MAX_B) return fail(LINETR_E_ARG, "detect_debug_labels: B=%d outside 1..%d", B, 2 * DET_MAX_B);
  if (H < 1 || W < 1 || H > DET_MAX_DIM || W > DET_MAX_DIM) return fail(LINETR_E_ARG, "detect_debug_labels: H=%d W=%d outside 1..%d", H, W, DET_MAX_DIM);
  if (!d_buckets || !d_labels || !d_workspace) return fail(LINETR_E_ARG, "detect_debug_labels: null pointer");
  if (((uintptr_t)d_labels & 3) || ((uintptr_t)d_workspace & 3)) return fail(LINETR_E_ARG, "detect_debug_labels: misaligned rows (labels and workspace 4 bytes)");
  if (workspace_bytes < (int64_t)B * H * W * 4) return fail(LINETR_E_ARG, "detect_debug_labels: workspace too small (need %lld)", (long long)B * H * W * 4);
  if (h) LT_HIP(hipSetDevice(h->device));
  return det_label(h, d_buckets, B, H, W, (int32_t*)d_workspace, d_labels, nullptr, nullptr, (hipStream_t)stream);
}

extern "C" int linetr_detect_debug_gradient(LinetrHandle* h, const void* d_images, int32_t images_are_float, int32_t B, int32_t H, int32_t W,
                                            const LinetrDetectConfig* cfg, int32_t octave, int32_t* d_m2, int8_t* d_bucket_a, int8_t* d_bucket_b,
                                            void* d_workspace, int64_t workspace_bytes, void* stream) {
  if (int e = det_dims_ok("detect_debug_gradient", B, H, W)) return e;
  if (int e = det_config_ok("detect_debug_gradient", cfg)) return e;
  if (octave < 0 || octave >= cfg->n_octaves) return fail(LINETR_E_ARG, "detect_debug_gradient: octave %d outside 0..%d", octave, cfg->n_octaves - 1);
  if (!d_images || !d_m2 || !d_bucket_a || !d_bucket_b || !d_workspace) return fail(LINETR_E_ARG, "detect_debug_gradient: null pointer");
  if (images_are_float != 0 && images_are_float != 1) return fail(LINETR_E_ARG, "detect_debug_gradient: images_are_float %d is neither 0 nor 1", images_are_float);
  if ((images_are_float && ((uintptr_t)d_images & 3)) || ((uintptr_t)d_m2 & 3) || ((uintptr_t)d_workspace & 255))
    return fail(LINETR_E_ARG, "detect_debug_gradient: misaligned rows (float32 images and m2 4, workspace 256 bytes)");
  DetLayout L = det_layout(B, H, W, cfg->n_octaves);
  if (workspace_bytes < L.total) return fail(LINETR_E_ARG, "detect_debug_gradient: workspace too small (need %lld)", (long long)L.total);
  det_bind(L, cfg->n_octaves, d_workspace);
  if (h) LT_HIP(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  if (int e = det_pyramid(h, d_images, images_are_float, B, L, octave + 1, st)) return e;
  const DetOct& o = L.oct[octave];
  if (o.Hc == 0) return LINETR_OK;      // an octave without cells: nothing to write
  return det_gradient(h, o, B, cfg->grad_threshold, d_m2, d_bucket_a, d_bucket_b, st);
}
