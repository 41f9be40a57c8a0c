// liblinetr_hip.so, translation unit 5 of 6: the image front end.  The native SuperPoint encoder (C ABI in include/linetr_hip.h; kernels
// in lt_spconv.h): inference only, float32 in and out, channel-last inside, deterministic.  The two dense-map entry points that consume
// its rows (linetr_superpoint_heads_rows) live next to linetr_superpoint_heads in linetr_match.hip.  In front of it the homography views
// of the dataset builder (lt_warp.h): linetr_warp_images and linetr_mask_erode.
#include <algorithm>

#include "lt_handle.h"
#include "lt_spconv.h"
#include "lt_warp.h"

using namespace lt;

namespace {

bool there16(const void* p) { return p && aligned16(p); }   // a required tensor: present and 16-byte aligned
constexpr int SP_MAX_DIM = 32768, SP_MAX_B = 65535;    // grid.z; tiles and pixel counts of one image stay far inside 2^31

// the (Cin, Cout) pairs of the encoder's 3x3 layers; 128 -> 512 is convPa | convDa as one launch
bool sp_pair_ok(int cin, int cout) {
  return (cin == 64 && (cout == 64 || cout == 128)) || (cin == 128 && (cout == 128 || cout == 256 || cout == 512));
}

int64_t sp_pack_floats(int cin, int cout_packed, int taps) { return (int64_t)cin * taps * cout_packed; }

template <int CIN, int CT, int KS, bool POOL>
void sp_launch_t(const SpConvArgs& a, int B, hipStream_t st) {
  const dim3 grid((unsigned)(cdiv(a.H, SP_TH) * cdiv(a.W, SP_TW)), (unsigned)(a.cout_packed / CT), (unsigned)B);
  hipLaunchKernelGGL((sp_conv_kernel<CIN, CT, KS, POOL>), grid, dim3(256), 0, st, a);
}

// One layer.  The caller has validated the shape; an empty output (pooling a single row or column) launches nothing.
int sp_conv_launch(LinetrHandle* h, const char* name, const SpConvArgs& a, int B, int cin, int ks, int pool, hipStream_t st) {
  const int Ho = pool ? a.H / 2 : a.H, Wo = pool ? a.W / 2 : a.W;
  if (B == 0 || Ho == 0 || Wo == 0) return LINETR_OK;
  const double px = (double)B * a.H * a.W;
  ProfScope ps(h, st, name, 2.0 * px * cin * ks * ks * a.cout_packed, 4.0 * (px * cin + (double)B * Ho * Wo * a.cout_store));
  if (ks == 1 && cin == 256) sp_launch_t<256, 128, 1, false>(a, B, st);
  else if (ks == 3 && cin == 64 && a.cout_packed == 64) pool ? sp_launch_t<64, 64, 3, true>(a, B, st) : sp_launch_t<64, 64, 3, false>(a, B, st);
  else if (ks == 3 && cin == 64) pool ? sp_launch_t<64, 128, 3, true>(a, B, st) : sp_launch_t<64, 128, 3, false>(a, B, st);
  else if (ks == 3 && cin == 128) pool ? sp_launch_t<128, 128, 3, true>(a, B, st) : sp_launch_t<128, 128, 3, false>(a, B, st);
  else return fail(LINETR_E_ARG, "%s: no kernel for Cin=%d k=%d", name, cin, ks);
  LT_LAUNCH_CHECK();
  return LINETR_OK;
}

int sp_pack_launch(const float* src, int cout_src, int cin, int taps, float* dst, int cout_packed, int cout_off, hipStream_t st) {
  const int64_t n = (int64_t)cout_src * cin * taps;
  hipLaunchKernelGGL(sp_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, src, cout_src, cin, taps, dst, cout_packed, cout_off);
  LT_LAUNCH_CHECK();
  return LINETR_OK;
}

int sp_conv1a_launch(LinetrHandle* h, const float* img, int B, int H, int W, const float* w, const float* b, float* y, hipStream_t st) {
  const int64_t pixels = (int64_t)B * H * W;
  ProfScope ps(h, st, "sp_conv1a", 2.0 * pixels * 9 * 64, 4.0 * pixels * 65);
  hipLaunchKernelGGL(sp_conv1a_kernel, dim3((unsigned)((pixels + 15) / 16)), dim3(256), 0, st, img, w, b, y, H, W, pixels);
  LT_LAUNCH_CHECK();
  return LINETR_OK;
}

// the eight 3x3 layers behind conv1a, in order; the last is convPa | convDa
struct SpLayer { const char* name; int cin, cout, pool; };
constexpr SpLayer SP_LAYERS[8] = {{"sp_conv1b", 64, 64, 1},   {"sp_conv2a", 64, 64, 0},   {"sp_conv2b", 64, 64, 1},   {"sp_conv3a", 64, 128, 0},
                                  {"sp_conv3b", 128, 128, 1}, {"sp_conv4a", 128, 128, 0}, {"sp_conv4b", 128, 128, 0}, {"sp_convPaDa", 128, 512, 0}};
constexpr int SP_PB_PACKED = 128;    // convPb's 65 outputs padded with zero weights to the 128-channel tile; the padding is never stored

// workspace of linetr_sp_encoder_forward: two buffers the layers alternate between
struct SpLayout { int64_t o_a, o_b, total; };
SpLayout sp_layout(int B, int H, int W) {
  SpLayout L{};
  Carve c;
  L.o_a = c.take(sz_mul(B, H, W, 64 * 4));                   // conv1a's output; every later "a" layer and the [cells, 512] rows fit
  L.o_b = c.take(sz_mul(B, H / 2, W / 2, 64 * 4));       // conv1b's pooled output; every later pooled map and conv4b's fit
  L.total = c.o;
  return L;
}
}  // namespace

struct LinetrSpEncoder {
  int device = 0;
  float* arena = nullptr;
  float *w1a = nullptr, *b1a = nullptr;      // conv1a in state_dict layout
  float *w[8] = {}, *b[8] = {};              // packed 3x3 layers (SP_LAYERS)
  float *wPb = nullptr, *bPb = nullptr, *wDb = nullptr, *bDb = nullptr;
  bool has_weights = false;
};

extern "C" int linetr_sp_conv3x3_tile(int32_t* tile_h, int32_t* tile_w) {
  if (!tile_h || !tile_w) return fail(LINETR_E_ARG, "sp_conv3x3_tile: null pointer");
  *tile_h = SP_TH;
  *tile_w = SP_TW;
  return LINETR_OK;
}

extern "C" int64_t linetr_sp_conv3x3_pack_bytes(int32_t Cin, int32_t Cout) { return sp_pair_ok(Cin, Cout) ? sp_pack_floats(Cin, Cout, 9) * 4 : 0; }

extern "C" int linetr_sp_conv3x3_pack(const float* d_w, int32_t Cin, int32_t Cout, float* d_packed, void* stream) {
  if (!sp_pair_ok(Cin, Cout)) return fail(LINETR_E_ARG, "sp_conv3x3_pack: unsupported layer %d -> %d", Cin, Cout);
  if (!there16(d_w) || !there16(d_packed)) return fail(LINETR_E_ARG, "sp_conv3x3_pack: a NULL or misaligned pointer");
  return sp_pack_launch(d_w, Cout, Cin, 9, d_packed, Cout, 0, (hipStream_t)stream);
}

extern "C" int linetr_sp_conv3x3(LinetrHandle* h, const float* d_x, int32_t B, int32_t H, int32_t W, int32_t Cin, const float* d_packed_w,
                                 const float* d_bias, int32_t Cout, int32_t pool, float* d_y, void* stream) {
  if (B < 1 || B > SP_MAX_B || H < 1 || W < 1 || H > SP_MAX_DIM || W > SP_MAX_DIM) return fail(LINETR_E_ARG, "sp_conv3x3: bad shape B=%d H=%d W=%d", B, H, W);
  if (!sp_pair_ok(Cin, Cout)) return fail(LINETR_E_ARG, "sp_conv3x3: unsupported layer %d -> %d", Cin, Cout);
  if (pool < 0 || pool > 1) return fail(LINETR_E_ARG, "sp_conv3x3: pool %d outside 0..1", pool);
  if (!there16(d_x) || !there16(d_packed_w) || !there16(d_bias) || !there16(d_y)) return fail(LINETR_E_ARG, "sp_conv3x3: a NULL or misaligned pointer");
  if (h) LT_HIP(hipSetDevice(h->device));
  SpConvArgs a{d_x, Cin, d_packed_w, d_bias, d_y, Cout, H, W, Cout, Cout, 1};
  return sp_conv_launch(h, "sp_conv3x3", a, B, Cin, 3, pool, (hipStream_t)stream);
}

extern "C" int linetr_sp_conv1a(LinetrHandle* h, const float* d_image, int32_t B, int32_t H, int32_t W, const float* d_w, const float* d_bias,
                                float* d_y, void* stream) {
  if (B < 1 || B > SP_MAX_B || H < 1 || W < 1 || H > SP_MAX_DIM || W > SP_MAX_DIM) return fail(LINETR_E_ARG, "sp_conv1a: bad shape B=%d H=%d W=%d", B, H, W);
  if (!there16(d_image) || !there16(d_w) || !there16(d_bias) || !there16(d_y)) return fail(LINETR_E_ARG, "sp_conv1a: a NULL or misaligned pointer");
  if (h) LT_HIP(hipSetDevice(h->device));
  return sp_conv1a_launch(h, d_image, B, H, W, d_w, d_bias, d_y, (hipStream_t)stream);
}

extern "C" int linetr_sp_encoder_create(int32_t device, LinetrSpEncoder** out) {
  if (!out) return fail(LINETR_E_ARG, "sp_encoder_create: null output");
  *out = nullptr;
  LT_HIP(hipSetDevice(device));
  Carve c;
  int64_t ow[8], ob[8];
  const int64_t o1w = c.take(64 * 9 * 4), o1b = c.take(64 * 4);
  for (int i = 0; i < 8; ++i) { ow[i] = c.take(sp_pack_floats(SP_LAYERS[i].cin, SP_LAYERS[i].cout, 9) * 4); ob[i] = c.take(SP_LAYERS[i].cout * 4); }
  const int64_t oPw = c.take(sp_pack_floats(256, SP_PB_PACKED, 1) * 4), oPb = c.take(SP_PB_PACKED * 4);
  const int64_t oDw = c.take(sp_pack_floats(256, 256, 1) * 4), oDb = c.take(256 * 4);
  char* base = nullptr;
  LT_HIP(hipMalloc((void**)&base, (size_t)c.o));
  auto* e = new LinetrSpEncoder;
  e->device = device;
  e->arena = (float*)base;
  e->w1a = (float*)(base + o1w); e->b1a = (float*)(base + o1b);
  for (int i = 0; i < 8; ++i) { e->w[i] = (float*)(base + ow[i]); e->b[i] = (float*)(base + ob[i]); }
  e->wPb = (float*)(base + oPw); e->bPb = (float*)(base + oPb);
  e->wDb = (float*)(base + oDw); e->bDb = (float*)(base + oDb);
  *out = e;
  return LINETR_OK;
}

extern "C" void linetr_sp_encoder_destroy(LinetrSpEncoder* enc) {
  if (!enc) return;
  (void)hipFree(enc->arena);
  delete enc;
}

extern "C" int linetr_sp_encoder_set_weights(LinetrSpEncoder* enc, const float* const* d_weights, const float* const* d_biases, void* stream) {
  if (!enc || !d_weights || !d_biases) return fail(LINETR_E_ARG, "sp_encoder_set_weights: null pointer");
  for (int i = 0; i < 12; ++i)
    if (!there16(d_weights[i]) || !there16(d_biases[i])) return fail(LINETR_E_ARG, "sp_encoder_set_weights: tensor %d is NULL or misaligned", i);
  LT_HIP(hipSetDevice(enc->device));
  hipStream_t st = (hipStream_t)stream;
  auto copy = [&](float* dst, const float* src, int n) { return hipMemcpyAsync(dst, src, (size_t)n * 4, hipMemcpyDeviceToDevice, st); };
  // state_dict order: conv1a conv1b conv2a conv2b conv3a conv3b conv4a conv4b convPa convPb convDa convDb
  LT_HIP(copy(enc->w1a, d_weights[0], 64 * 9));
  LT_HIP(copy(enc->b1a, d_biases[0], 64));
  for (int i = 0; i < 7; ++i) {
    if (int e = sp_pack_launch(d_weights[1 + i], SP_LAYERS[i].cout, SP_LAYERS[i].cin, 9, enc->w[i], SP_LAYERS[i].cout, 0, st)) return e;
    LT_HIP(copy(enc->b[i], d_biases[1 + i], SP_LAYERS[i].cout));
  }
  // convPa | convDa: channels 0..255 / 256..511 of one 128 -> 512 layer
  if (int e = sp_pack_launch(d_weights[8], 256, 128, 9, enc->w[7], 512, 0, st)) return e;
  if (int e = sp_pack_launch(d_weights[10], 256, 128, 9, enc->w[7], 512, 256, st)) return e;
  LT_HIP(copy(enc->b[7], d_biases[8], 256));
  LT_HIP(copy(enc->b[7] + 256, d_biases[10], 256));
  LT_HIP(hipMemsetAsync(enc->wPb, 0, (size_t)sp_pack_floats(256, SP_PB_PACKED, 1) * 4, st));
  LT_HIP(hipMemsetAsync(enc->bPb, 0, SP_PB_PACKED * 4, st));
  if (int e = sp_pack_launch(d_weights[9], 65, 256, 1, enc->wPb, SP_PB_PACKED, 0, st)) return e;
  LT_HIP(copy(enc->bPb, d_biases[9], 65));
  if (int e = sp_pack_launch(d_weights[11], 256, 256, 1, enc->wDb, 256, 0, st)) return e;
  LT_HIP(copy(enc->bDb, d_biases[11], 256));
  enc->has_weights = true;
  return LINETR_OK;
}

extern "C" int64_t linetr_sp_encoder_workspace_bytes(int32_t B, int32_t H, int32_t W) {
  if (B < 1 || B > SP_MAX_B || H < 8 || W < 8 || H > SP_MAX_DIM || W > SP_MAX_DIM) return 0;   // what linetr_sp_encoder_forward refuses
  return sz_answer(sp_layout(B, H, W).total);
}

extern "C" int linetr_sp_encoder_forward(LinetrSpEncoder* enc, const float* d_image, int32_t B, int32_t H, int32_t W, float* d_score_rows,
                                         float* d_desc_rows, float* d_feat, void* d_workspace, int64_t workspace_bytes, void* stream) {
  if (!enc || !enc->has_weights) return fail(LINETR_E_ARG, "sp_encoder_forward: an encoder without weights");
  if (B < 1 || B > SP_MAX_B || H < 8 || W < 8 || H > SP_MAX_DIM || W > SP_MAX_DIM) return fail(LINETR_E_ARG, "sp_encoder_forward: bad shape B=%d H=%d W=%d", B, H, W);
  if (!there16(d_image) || !there16(d_score_rows) || !there16(d_desc_rows) || !there16(d_workspace) || (d_feat && !there16(d_feat)))
    return fail(LINETR_E_ARG, "sp_encoder_forward: a NULL or misaligned pointer");
  const SpLayout L = sp_layout(B, H, W);
  if (workspace_bytes < L.total) return fail(LINETR_E_ARG, "sp_encoder_forward: workspace too small (need %lld)", (long long)L.total);
  LT_HIP(hipSetDevice(enc->device));
  hipStream_t st = (hipStream_t)stream;
  float* buf[2] = {(float*)((char*)d_workspace + L.o_a), (float*)((char*)d_workspace + L.o_b)};
  if (int e = sp_conv1a_launch(nullptr, d_image, B, H, W, enc->w1a, enc->b1a, buf[0], st)) return e;
  int h = H, w = W, cur = 0;
  for (int i = 0; i < 8; ++i) {
    const SpLayer& ly = SP_LAYERS[i];
    float* out = (i == 6 && d_feat) ? d_feat : buf[cur ^ 1];
    const float* in = (i == 7 && d_feat) ? d_feat : buf[cur];
    SpConvArgs a{in, ly.cin, enc->w[i], enc->b[i], out, ly.cout, h, w, ly.cout, ly.cout, 1};
    if (int e = sp_conv_launch(nullptr, ly.name, a, B, ly.cin, 3, ly.pool, st)) return e;
    if (ly.pool) { h /= 2; w /= 2; }
    cur ^= 1;
  }
  // the two 1x1 heads on the [cells, 512] rows: convPb reads channels 0..255 (convPa's), convDb channels 256..511 (convDa's)
  const float* rows = buf[cur];
  SpConvArgs pb{rows, 512, enc->wPb, enc->bPb, d_score_rows, LINETR_SP_SCORE_LD, h, w, SP_PB_PACKED, 65, 0};
  if (int e = sp_conv_launch(nullptr, "sp_convPb", pb, B, 256, 1, 0, st)) return e;
  SpConvArgs db{rows + 256, 512, enc->wDb, enc->bDb, d_desc_rows, 256, h, w, 256, 256, 0};
  return sp_conv_launch(nullptr, "sp_convDb", db, B, 256, 1, 0, st);
}

// =============================================================================================
// homography views: warped image batches with their valid masks, and the erosion of a mask (lt_warp.h)
// =============================================================================================

namespace {
// B, H, W, C positive, one image below 2^31 elements (plane offsets are ints), extents inside the grid limits
int view_dims_ok(const char* who, int64_t B, int64_t C, int64_t H, int64_t W) {
  if (B < 1 || C < 1 || H < 1 || W < 1) return fail(LINETR_E_ARG, "%s: bad shape B=%lld C=%lld H=%lld W=%lld", who, (long long)B, (long long)C, (long long)H, (long long)W);
  if (H > SP_MAX_DIM || W > SP_MAX_DIM || H * W * C >= ((int64_t)1 << 31))
    return fail(LINETR_E_ARG, "%s: H * W * C = %lld x %lld x %lld at or beyond 2^31 elements (or an extent above %d)", who, (long long)H, (long long)W, (long long)C, SP_MAX_DIM);
  return LINETR_OK;
}
}  // namespace

extern "C" int linetr_warp_images(LinetrHandle* h, const float* d_src, int32_t B, int32_t C, int32_t H, int32_t W, const double* h_mat,
                                  int32_t mode, float* d_dst, uint8_t* d_valid, void* stream) {
  // every refusal comes before the first launch
  if (int e = view_dims_ok("warp_images", B, C, H, W)) return e;
  if (!d_src || !d_dst || !h_mat) return fail(LINETR_E_ARG, "warp_images: null pointer");
  if (mode != 0 && mode != 1) return fail(LINETR_E_ARG, "warp_images: mode %d is neither 0 (bilinear) nor 1 (nearest)", mode);
  if (((uintptr_t)d_src | (uintptr_t)d_dst) & 3) return fail(LINETR_E_ARG, "warp_images: a float tensor that is not 4-byte aligned");
  if (d_src == d_dst) return fail(LINETR_E_ARG, "warp_images: in-place operation (d_dst == d_src)");
  for (int64_t i = 0; i < (int64_t)B * 9; ++i)
    if (!std::isfinite(h_mat[i])) return fail(LINETR_E_ARG, "warp_images: matrix %lld has a non-finite entry", (long long)(i / 9));
  if (h) LT_HIP(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  const int vec = W % 4 == 0 && aligned16(d_dst) && (!d_valid || ((uintptr_t)d_valid & 3) == 0);
  const double px = (double)B * H * W;
  ProfScope ps(h, st, "warp_images", 0, px * (8.0 * C + (d_valid ? 1 : 0)));
  for (int first = 0; first < B; first += WARP_CHUNK) {
    const int count = std::min(WARP_CHUNK, B - first);
    WarpMats mats{};
    memcpy(mats.m, h_mat + (int64_t)first * 9, (size_t)count * 9 * sizeof(double));
    const dim3 grid((unsigned)cdiv(W, WARP_TW), (unsigned)cdiv(H, WARP_TH), (unsigned)count);
    if (mode == 0) hipLaunchKernelGGL(warp_kernel<0>, grid, dim3(256), 0, st, d_src, mats, first, C, H, W, vec, d_dst, d_valid);
    else hipLaunchKernelGGL(warp_kernel<1>, grid, dim3(256), 0, st, d_src, mats, first, C, H, W, vec, d_dst, d_valid);
    LT_LAUNCH_CHECK();
  }
  return LINETR_OK;
}

extern "C" int linetr_warp_tile(int32_t* tile_h, int32_t* tile_w, int32_t* erode_tile_h, int32_t* erode_tile_w) {
  if (!tile_h || !tile_w || !erode_tile_h || !erode_tile_w) return fail(LINETR_E_ARG, "warp_tile: null pointer");
  *tile_h = WARP_TH;
  *tile_w = WARP_TW;
  *erode_tile_h = ERODE_TH;
  *erode_tile_w = ERODE_TW;
  return LINETR_OK;
}

extern "C" int linetr_mask_erode(LinetrHandle* h, const uint8_t* d_mask, int32_t B, int32_t H, int32_t W, int32_t radius, uint8_t* d_out,
                                 void* stream) {
  if (int e = view_dims_ok("mask_erode", B, 1, H, W)) return e;
  if (B > SP_MAX_B) return fail(LINETR_E_ARG, "mask_erode: B=%d above %d", B, SP_MAX_B);
  if (!d_mask || !d_out) return fail(LINETR_E_ARG, "mask_erode: null pointer");
  if (radius < 0 || radius > ERODE_MAX_R) return fail(LINETR_E_ARG, "mask_erode: radius %d outside 0..%d", radius, ERODE_MAX_R);
  const int64_t bytes = (int64_t)B * H * W;
  if (d_out < d_mask + bytes && d_mask < d_out + bytes) return fail(LINETR_E_ARG, "mask_erode: in-place operation (d_out overlaps d_mask)");
  if (h) LT_HIP(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  const int vec = W % 4 == 0 && ((uintptr_t)d_out & 3) == 0;
  ProfScope ps(h, st, "mask_erode", 0, 2.0 * bytes);
  hipLaunchKernelGGL(erode_kernel, dim3((unsigned)cdiv(W, ERODE_TW), (unsigned)cdiv(H, ERODE_TH), (unsigned)B), dim3(256), 0, st, d_mask, H, W,
                     radius, vec, d_out);
  LT_LAUNCH_CHECK();
  return LINETR_OK;
}
