// Key-line -> sub-line tokenisation, descriptor sampling and score gather on the device.
// Replaces the Python double loop of models/line_process.py:100-196 (line_tokenizer),
// :86-98 (sample_descriptors) and :174-179 (score gather).
#pragma once
#include "lt_common.h"

namespace lt {

// One image of a ragged batch (linetr_describe_ragged: every image at its own size): what the kernels of the front of the pipeline read
// from their arguments when all images have one size.  The table is built on the host and lives in the call's workspace.
struct RaggedImage {
  const void* nhwc;     // the image's channel-last descriptor map: the caller's own, or its copy in the workspace (the call's element type)
  const float* score;   // its score map [height][width]
  const void* nchw;     // the caller's [256][Hc][Wc] map the layout pass reads (NULL: the feed is channel-last)
  int height, width, Hc, Wc;
  double td;            // token_distance
  double clip_x, clip_y;   // end-point clip (width - 0.6, height - 0.6)
};                      // 64 bytes
static_assert(sizeof(RaggedImage) == 64, "RaggedImage is copied as 64-byte entries");

// ---------------------------------------------------------------------------------------------
// NCHW -> NHWC copy of the dense descriptor map so that each bilinear tap is one coalesced 1 KiB
// row (SuperPoint emits [1,256,H/8,W/8], models/superpoint.py:193).  32x32 LDS-tiled transpose.
// grid (P/64 ceil, C/64, B), block 256
// ---------------------------------------------------------------------------------------------
// one block's 64 channels x 64 positions of ONE image: src [C][P] -> dst [P][C]
__device__ __forceinline__ void nchw_to_nhwc_tile(const float* src, float* dst, int C, int P, int p0, int c0) {
  // 64 channels x 64 positions per block, dwordx4 on both sides: reads 16 B along p (NCHW rows), writes 16 B along c
  // (NHWC rows).  LDS tile [64 c][64 p + 1]: the odd stride keeps the 4-way column gather conflict-free.
  __shared__ float tile[64][65];
  const int tid = threadIdx.x;
  {
    const int pq = (tid & 15) * 4;          // 16 threads cover 64 positions
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = (tid >> 4) + i * 16;
      const float* row = src + (int64_t)(c0 + c) * P + p0 + pq;
      f32x4 v;
      if (p0 + pq + 3 < P && (((uintptr_t)row) & 15) == 0) v = *reinterpret_cast<const f32x4*>(row);
      else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = p0 + pq + k < P ? row[k] : 0.f;
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) tile[c][pq + k] = v[k];
    }
  }
  __syncthreads();
  {
    const int cq = (tid & 15) * 4;          // 16 threads cover 64 channels of one position
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int p = (tid >> 4) + i * 16;
      if (p0 + p < P) {
        f32x4 v;
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = tile[cq + k][p];
        *reinterpret_cast<f32x4*>(dst + (int64_t)(p0 + p) * C + c0 + cq) = v;
      }
    }
  }
}

static __global__ __launch_bounds__(256) void nchw_to_nhwc_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                           int C, int P) {
  const int b = blockIdx.z;
  nchw_to_nhwc_tile(in + (int64_t)b * C * P, out + (int64_t)b * C * P, C, P, blockIdx.x * 64, blockIdx.y * 64);
}

// ragged: image blockIdx.z has its own P = Hc * Wc (an odd P leaves every other row off the 16-byte grid: the aligned and the
// unaligned load are chosen row by row, as above); grid.x covers the largest image, the blocks past a smaller one leave
static __global__ __launch_bounds__(256) void nchw_to_nhwc_ragged_kernel(const RaggedImage* __restrict__ tab, int C) {
  const RaggedImage im = tab[blockIdx.z];
  const int P = im.Hc * im.Wc, p0 = blockIdx.x * 64;
  if (p0 >= P) return;
  nchw_to_nhwc_tile((const float*)im.nchw, (float*)const_cast<void*>(im.nhwc), C, P, p0, blockIdx.y * 64);
}

// The same pass on a half map (float16 or bfloat16: a transpose moves 2-byte elements and never looks into them): 8 bytes on both sides,
// halves into a half channel-last scratch.  A half NCHW map may lie at any 2-byte address: the 8-byte load is chosen row by row.
// LDS tile [64 c][64 p + 2] halves: rows 33 dwords apart.
__device__ __forceinline__ void nchw_to_nhwc_tile(const uint16_t* src, uint16_t* dst, int C, int P, int p0, int c0) {
  __shared__ uint16_t tile[64][66];
  const int tid = threadIdx.x;
  {
    const int pq = (tid & 15) * 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = (tid >> 4) + i * 16;
      const uint16_t* row = src + (int64_t)(c0 + c) * P + p0 + pq;
      u16x4 v;
      if (p0 + pq + 3 < P && (((uintptr_t)row) & 7) == 0) v = *reinterpret_cast<const u16x4*>(row);
      else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = p0 + pq + k < P ? row[k] : (uint16_t)0;
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) tile[c][pq + k] = v[k];
    }
  }
  __syncthreads();
  {
    const int cq = (tid & 15) * 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int p = (tid >> 4) + i * 16;
      if (p0 + p < P) {
        u16x4 v;
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = tile[cq + k][p];
        *reinterpret_cast<u16x4*>(dst + (int64_t)(p0 + p) * C + c0 + cq) = v;
      }
    }
  }
}

static __global__ __launch_bounds__(256) void nchw_to_nhwc_half_kernel(const uint16_t* __restrict__ in, uint16_t* __restrict__ out,
                                                                int C, int P) {
  const int b = blockIdx.z;
  nchw_to_nhwc_tile(in + (int64_t)b * C * P, out + (int64_t)b * C * P, C, P, blockIdx.x * 64, blockIdx.y * 64);
}

static __global__ __launch_bounds__(256) void nchw_to_nhwc_half_ragged_kernel(const RaggedImage* __restrict__ tab, int C) {
  const RaggedImage im = tab[blockIdx.z];
  const int P = im.Hc * im.Wc, p0 = blockIdx.x * 64;
  if (p0 >= P) return;
  nchw_to_nhwc_tile((const uint16_t*)im.nchw, (uint16_t*)const_cast<void*>(im.nhwc), C, P, p0, blockIdx.y * 64);
}

// ---------------------------------------------------------------------------------------------
// per key-line: float32 copies of klines/length/angles (models/line_process.py:182-184, with the
// end-point clip of :114-116 already applied) and the sub-line -> key-line maps.
// ---------------------------------------------------------------------------------------------
// one key-line's row of the three arrays (also the rows of lt_fixedsize.h)
__device__ __forceinline__ void kline_row(const LinetrLineRec& r, double wclip, double hclip, float* __restrict__ kline,
                                          float* __restrict__ length, float* __restrict__ angle) {
  kline[0] = (float)r.sp[0];
  kline[1] = (float)r.sp[1];
  kline[2] = (float)fmin(r.ep[0], wclip);
  kline[3] = (float)fmin(r.ep[1], hclip);
  *length = (float)r.length;
  angle[0] = (float)r.angle[0];
  angle[1] = (float)r.angle[1];
}

__device__ __forceinline__ void line_fill_one(const LinetrLineRec& r, int k, double wclip, double hclip, float* klines, float* length,
                                              float* angles, int* sub2line_g, int* sub2line_l) {
  if (klines) kline_row(r, wclip, hclip, klines + k * 4, length + k, angles + k * 2);
  for (int s = 0; s < r.n_sub; ++s) {
    sub2line_g[r.first_sub + s] = k;
    if (sub2line_l) sub2line_l[r.first_sub + s] = r.line_local;
  }
}

static __global__ void line_fill_kernel(const LinetrLineRec* __restrict__ recs, int K, double wclip, double hclip,
                                 float* __restrict__ klines, float* __restrict__ length,
                                 float* __restrict__ angles, int* __restrict__ sub2line_g,
                                 int* __restrict__ sub2line_l) {
  int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= K) return;
  const LinetrLineRec r = recs[k];
  line_fill_one(r, k, wclip, hclip, klines, length, angles, sub2line_g, sub2line_l);
}

// ragged: the end-point clip is the key-line's own image's
static __global__ void line_fill_ragged_kernel(const LinetrLineRec* __restrict__ recs, int K, const RaggedImage* __restrict__ tab,
                                        float* __restrict__ klines, float* __restrict__ length, float* __restrict__ angles,
                                        int* __restrict__ sub2line_g, int* __restrict__ sub2line_l) {
  int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= K) return;
  const LinetrLineRec r = recs[k];
  line_fill_one(r, k, tab[r.image].clip_x, tab[r.image].clip_y, klines, length, angles, sub2line_g, sub2line_l);
}

// mat_klines2sublines of a small batch: where every image's [K_i][N_i] block starts (floats), its row length and the batch-wide index
// of its first sub-line.  Travels in the kernel arguments.
constexpr int K2S_MAX_IMAGES = 8;
struct K2sImage { int64_t off; int n_sub; int sub_base; };
struct K2sTable { K2sImage img[K2S_MAX_IMAGES]; };

// a key-line's entry of mat_klines2sublines over its own sub-lines: Python's 1 / num is a float64 quotient stored as float32
__device__ __forceinline__ float k2s_weight(const LinetrLineRec& r) { return (float)(1.0 / (double)r.n_sub); }

// point at arclength `d` from sp along sp->ep in the reference's slope form, float64, no FMA
// contraction (models/line_process.py:43-57).
__device__ __forceinline__ void walk_along(const double sp[2], const double ep[2], double d, double& x, double& y) {
#pragma clang fp contract(off)
  const double vx = ep[0] - sp[0], vy = ep[1] - sp[1];
  double dx, dy;
  if (vx != 0.0) {
    const double m = vy / vx;
    dx = sqrt(d * d / (1.0 + m * m));
    dy = m * dx;
  } else {
    dx = 0.0;
    dy = vy > 0.0 ? d : -d;
  }
  x = dx + sp[0];
  y = dy + sp[1];
}

// One sub-line's rows of the tokeniser's tensors: sub-line `j` of key-line `r`, written at row `n` of every output (the tokeniser: the
// batch-wide sub-line index; lt_fixedsize.h: row b * max_sublines + j' of the fixed-size sample).  One 64-thread block.
__device__ __forceinline__ void tokenize_subline(
    const LinetrLineRec& r, int j, int n, double td, int T, int height, int width, double clip_x, double clip_y,
    const float* __restrict__ dense_score, float* __restrict__ sublines, float* __restrict__ pnt, float* __restrict__ mask,
    float* __restrict__ resp, float* __restrict__ angle_sub, float* __restrict__ score, float* __restrict__ cpnt,
    float* __restrict__ cscore) {
#pragma clang fp contract(off)
  // end-point clip of line_process.py:115-116: the limits come from the `image_shape` ARGUMENT of line_tokenizer (width - 0.6,
  // height - 0.6), which need not be the score map's shape (the dataset builder passes (640, 480) for a 480 x 640 image)
  const double epc[2] = {fmin(r.ep[0], clip_x), fmin(r.ep[1], clip_y)};
  for (int t = threadIdx.x; t < T; t += 64) {
    const int ti = j * T + t;
    double x = 0.0, y = 0.0;
    float mk = 0.f;
    if (ti < r.n_tok - 1) {
      walk_along(r.sp, r.ep, (double)ti * td, x, y);  // :110-113
      mk = 1.f;
    } else if (ti == r.n_tok - 1) {
      x = epc[0];                                      // :114-117
      y = epc[1];
      mk = 1.f;
    }
    const float fx = (float)x, fy = (float)y;          // :157 .float()
    const int64_t o = (int64_t)n * T + t;
    if (pnt) { pnt[o * 2 + 0] = fx; pnt[o * 2 + 1] = fy; }
    if (mask) mask[(int64_t)n * (T + 1) + 1 + t] = mk;
    // score gather :174-179 -- torch.round (half to even), clip to the map, index [y][x]
    int ix = (int)rintf(fx), iy = (int)rintf(fy);
    ix = ix < width - 1 ? ix : width - 1;
    iy = iy < height - 1 ? iy : height - 1;
    ix = ix < 0 ? 0 : ix;   // negative coordinates cannot occur after remove_borders; guard the load anyway
    iy = iy < 0 ? 0 : iy;
    const float sc = dense_score[(int64_t)r.image * height * width + (int64_t)iy * width + ix];
    if (score) score[o] = sc;
    if (cpnt && mk != 0.f) {  // compact list of real tokens (fused path)
      const int64_t c = (int64_t)r.first_tok + ti;
      cpnt[c * 2 + 0] = fx;
      cpnt[c * 2 + 1] = fy;
      cscore[c] = sc;
    }
  }
  if (threadIdx.x == 0) {
    if (mask) mask[(int64_t)n * (T + 1)] = 1.f;  // CLS slot :135
    double s[2], e[2];
    if (j == 0) { s[0] = r.sp[0]; s[1] = r.sp[1]; }
    else walk_along(r.sp, r.ep, (double)(j * T - 1) * td, s[0], s[1]);        // :125-128
    if (j == r.n_sub - 1) { e[0] = epc[0]; e[1] = epc[1]; }
    else walk_along(r.sp, r.ep, (double)((j + 1) * T - 1) * td, e[0], e[1]);
    sublines[(int64_t)n * 4 + 0] = (float)s[0];
    sublines[(int64_t)n * 4 + 1] = (float)s[1];
    sublines[(int64_t)n * 4 + 2] = (float)e[0];
    sublines[(int64_t)n * 4 + 3] = (float)e[1];
    const double dx = e[0] - s[0], dy = e[1] - s[1];
    const double geo = sqrt(dx * dx + dy * dy);                               // :148-149
    resp[n] = (float)(geo / (td * (double)T));
    angle_sub[(int64_t)n * 2 + 0] = (float)r.angle[0];                        // :151
    angle_sub[(int64_t)n * 2 + 1] = (float)r.angle[1];
  }
}

// The tokeniser's blocks past the sub-lines (block `x` of them), written once for both kernels below; score_of(i) = image i's score map.
template <class ScoreOf>
__device__ __forceinline__ void tokenize_extra_block(int x, const LinetrLineRec* recs, float* cpnt, float* cscore, int n_pad_images,
                                                     int64_t first_pad, ScoreOf score_of, float* mat_k2s, const K2sTable& k2s) {
  const int pad_blocks = (n_pad_images + 63) / 64;
  if (x < pad_blocks) {
    // one shared padding token per image for the compact token list -- coordinate (0, 0), score
    // dense_score[img][0][0] (the reference pads with zeros and gathers the score at the rounded coordinate, line_process.py:174-179)
    const int i = x * 64 + threadIdx.x;
    if (i < n_pad_images) {
      cpnt[(first_pad + i) * 2 + 0] = 0.f;
      cpnt[(first_pad + i) * 2 + 1] = 0.f;
      cscore[first_pad + i] = *score_of(i);
    }
    return;
  }
  // one more block per key-line (calls of up to K2S_MAX_IMAGES images): its row of the image's mat_klines2sublines [K_i][N_i],
  // 1 / num_sublines over the key-line's own sub-lines and 0 elsewhere (line_process.py:160-165; Python's 1/num is a float64
  // quotient stored as float32)
  const int k = x - pad_blocks;
  const LinetrLineRec r = recs[k];
  const K2sImage im = k2s.img[r.image & (K2S_MAX_IMAGES - 1)];
  float* row = mat_k2s + im.off + (int64_t)r.line_local * im.n_sub;
  const float w = k2s_weight(r);
  const int j0 = r.first_sub - im.sub_base;
  for (int j = threadIdx.x; j < im.n_sub; j += 64) row[j] = (j >= j0 && j < j0 + r.n_sub) ? w : 0.f;
}

// ---------------------------------------------------------------------------------------------
// One 64-thread block per sub-line; thread t < T produces token t.
// ---------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(64) void tokenize_kernel(
    const LinetrLineRec* __restrict__ recs, const int* __restrict__ sub2line_g, int N, double td, int T,
    int height, int width, double clip_x, double clip_y, const float* __restrict__ dense_score, float* __restrict__ sublines,
    float* __restrict__ pnt, float* __restrict__ mask, float* __restrict__ resp,
    float* __restrict__ angle_sub, float* __restrict__ score, float* __restrict__ cpnt,
    float* __restrict__ cscore, int n_pad_images, int64_t first_pad, float* __restrict__ mat_k2s, const K2sTable k2s) {
#pragma clang fp contract(off)
  const int n = blockIdx.x;
  if (n >= N) {   // blocks past the sub-lines: the images' padding tokens, then (out.mat) the rows of mat_klines2sublines
    tokenize_extra_block(n - N, recs, cpnt, cscore, n_pad_images, first_pad,
                         [&](int i) { return dense_score + (int64_t)i * height * width; }, mat_k2s, k2s);
    return;
  }
  const LinetrLineRec r = recs[sub2line_g[n]];
  tokenize_subline(r, n - r.first_sub, n, td, T, height, width, clip_x, clip_y, dense_score, sublines, pnt, mask, resp, angle_sub, score,
                   cpnt, cscore);
}

// ragged: size, token distance, clip and score map come from the key-line's own table entry
static __global__ __launch_bounds__(64) void tokenize_ragged_kernel(
    const LinetrLineRec* __restrict__ recs, const int* __restrict__ sub2line_g, int N, int T, const RaggedImage* __restrict__ tab,
    float* __restrict__ sublines, float* __restrict__ pnt, float* __restrict__ mask, float* __restrict__ resp,
    float* __restrict__ angle_sub, float* __restrict__ score, float* __restrict__ cpnt, float* __restrict__ cscore, int n_pad_images,
    int64_t first_pad, float* __restrict__ mat_k2s, const K2sTable k2s) {
#pragma clang fp contract(off)
  const int n = blockIdx.x;
  if (n >= N) {
    tokenize_extra_block(n - N, recs, cpnt, cscore, n_pad_images, first_pad, [&](int i) { return tab[i].score; }, mat_k2s, k2s);
    return;
  }
  LinetrLineRec r = recs[sub2line_g[n]];
  const RaggedImage im = tab[r.image];
  r.image = 0;   // im.score is the map of this image alone: image 0 of a batch of one (nothing else below reads the field)
  tokenize_subline(r, n - r.first_sub, n, im.td, T, im.height, im.width, im.clip_x, im.clip_y, im.score, sublines, pnt, mask, resp,
                   angle_sub, score, cpnt, cscore);
}

// ---------------------------------------------------------------------------------------------
// sample_descriptors (models/line_process.py:86-98): bilinear grid_sample (zero padding) of the NHWC
// descriptor map + L2 normalisation.  One wave64 per token, lane = 4 channels (dwordx4, coalesced
// 1 KiB per tap).  fp32 arithmetic in the order PyTorch's CPU grid_sampler uses.
// ---------------------------------------------------------------------------------------------
// --- the same sampling split into "issue the 4 tap loads" and "finish", so a caller can keep the next
// token's loads in flight while it works on the current one -----------------------------------------------
template <class E> struct TapSetT { typename Elem<E>::raw4 v[4]; float w[4]; };   // nw, ne, sw, se values (as loaded) and weights
typedef TapSetT<float> TapSet;

// grid_sample's un-normalisation in the operation order of PyTorch's CPU kernel (the reference runs it on the CPU; its vectorised
// grid sampler computes (g + 1) * (size / 2) - 0.5 with ONE rounding -- the compiler contracts the multiply-add of its vector
// operators -- and (g + 1) * ((size - 1) / 2) with align_corners).  r06: established by matching torch 2.10's CPU output bit for bit
// on 20 000 points per map size (60 x 80 and 120 x 160 cells: 100 % identical samples with this form; the former
// ((g + 1) * size - 1) / 2 left 1-3 % of the samples up to 2e-6 off, 4e-6 after normalisation on 960 x 1280 images).
__device__ __forceinline__ float grid_unnormalize(float g, int size, int align_corners) {
#pragma clang fp contract(off)
  if (align_corners) return (g + 1.f) * ((float)(size - 1) / 2.f);
  return __builtin_fmaf(g + 1.f, (float)size / 2.f, -0.5f);
}

// Bilinear tap geometry of one point (sample_descriptors' grid arithmetic, models/line_process.py:86-98, and
// grid_sample's unnormalisation): 4 cell offsets (clamped, in cells) and weights (0 for taps outside the map: zero padding).
__device__ __forceinline__ void tap_coords(float px, float py, int Hc, int Wc, int align_corners, int (&off)[4],
                                           float (&wt)[4]) {
#pragma clang fp contract(off)
  const float s = 8.f;
  float gx = ((px - s / 2) + 0.5f) / ((float)Wc * s - s / 2 - 0.5f);
  float gy = ((py - s / 2) + 0.5f) / ((float)Hc * s - s / 2 - 0.5f);
  gx = gx * 2.f - 1.f;
  gy = gy * 2.f - 1.f;
  const float ix = grid_unnormalize(gx, Wc, align_corners), iy = grid_unnormalize(gy, Hc, align_corners);
  const float x_w = floorf(ix), y_n = floorf(iy);
  const float w = ix - x_w, e = 1.f - w, nn = iy - y_n, ss = 1.f - nn;
  const float wv[4] = {ss * e, ss * w, nn * e, nn * w};
  const int x0 = (int)x_w, y0 = (int)y_n;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int yy = y0 + (k >> 1), xx = x0 + (k & 1);
    const bool in = xx >= 0 && xx < Wc && yy >= 0 && yy < Hc;
    const int yc = min(max(yy, 0), Hc - 1), xc = min(max(xx, 0), Wc - 1);
    off[k] = yc * Wc + xc;
    wt[k] = in ? wv[k] : 0.f;
  }
}

// loads of the 4 taps (this lane's 4 channels); the address is always valid, out-of-map taps carry weight 0
template <class E>
__device__ __forceinline__ void taps_load(const E* __restrict__ nhwc_img, const int (&off)[4], const float (&wt)[4],
                                          int lane, TapSetT<E>& t) {
  const E* base = nhwc_img + lane * 4;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    t.v[k] = load_raw4(base + (int64_t)off[k] * D);
    t.w[k] = wt[k];
  }
}

template <class E>
__device__ __forceinline__ void taps_issue(float px, float py, const E* __restrict__ nhwc_img, int Hc, int Wc,
                                           int align_corners, int lane, TapSetT<E>& t) {
  int off[4];
  float wt[4];
  tap_coords(px, py, Hc, Wc, align_corners, off, wt);
  taps_load(nhwc_img, off, wt, lane, t);
}

// RCP = true: one division + 4 multiplies instead of 4 divisions (<= 1 ulp apart); only for consumers that never
// expose the sampled descriptor itself (the pooling kernel), the reference's desc_sublines keeps the exact form.
// (a half tap set is widened here, at its first use: the loads stay in flight until then)
template <bool RCP = false, class E>
__device__ __forceinline__ f32x4 taps_finish(const TapSetT<E>& t) {
#pragma clang fp contract(off)
  const f32x4 t0 = Elem<E>::widen(t.v[0]), t1 = Elem<E>::widen(t.v[1]), t2 = Elem<E>::widen(t.v[2]), t3 = Elem<E>::widen(t.v[3]);
  f32x4 o;
  float sq = 0.f;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    float v = t0[c] * t.w[0];                      // nw * w_nw, then one fused multiply-add per further tap: the CPU kernel's order
    v = __builtin_fmaf(t1[c], t.w[1], v);
    v = __builtin_fmaf(t2[c], t.w[2], v);
    v = __builtin_fmaf(t3[c], t.w[3], v);
    o[c] = v;
    sq += v * v;
  }
  sq = wave_sum(sq);
  const float nrm = fmaxf(sqrtf(sq), 1e-12f);
  if constexpr (RCP) {
    const float inv = 1.f / nrm;
#pragma unroll
    for (int c = 0; c < 4; ++c) o[c] = o[c] * inv;
  } else {
#pragma unroll
    for (int c = 0; c < 4; ++c) o[c] = o[c] / nrm;
  }
  return o;
}

// bilinear sample (zero padding) + L2 normalisation of one token; every lane of the wave returns its 4 channels
template <class E>
__device__ __forceinline__ f32x4 sample_one(float px, float py, const E* __restrict__ nhwc_img, int Hc, int Wc,
                                            int align_corners, int lane) {
#pragma clang fp contract(off)
  const float s = 8.f;
  // keypoints - s/2 + 0.5 ; /= (w*s - s/2 - 0.5) ; *2 - 1          (:88-92)
  float gx = ((px - s / 2) + 0.5f) / ((float)Wc * s - s / 2 - 0.5f);
  float gy = ((py - s / 2) + 0.5f) / ((float)Hc * s - s / 2 - 0.5f);
  gx = gx * 2.f - 1.f;
  gy = gy * 2.f - 1.f;
  const float ix = grid_unnormalize(gx, Wc, align_corners), iy = grid_unnormalize(gy, Hc, align_corners);
  const float x_w = floorf(ix), y_n = floorf(iy);
  const float w = ix - x_w, e = 1.f - w, nn = iy - y_n, ss = 1.f - nn;
  const float nw = ss * e, ne = ss * w, sw = nn * e, se = nn * w;
  const int x0 = (int)x_w, y0 = (int)y_n, x1 = x0 + 1, y1 = y0 + 1;
  const E* base = nhwc_img + lane * 4;
  auto tap = [&](int yy, int xx) -> f32x4 {
    if (xx < 0 || xx >= Wc || yy < 0 || yy >= Hc) return f32x4{0.f, 0.f, 0.f, 0.f};
    return Elem<E>::widen(load_raw4(base + ((int64_t)yy * Wc + xx) * D));
  };
  const f32x4 v_nw = tap(y0, x0), v_ne = tap(y0, x1), v_sw = tap(y1, x0), v_se = tap(y1, x1);
  f32x4 o;
  float sq = 0.f;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    float v = v_nw[c] * nw;                        // (nw_val * nw) + (ne_val * ne) + ... as the CPU kernel evaluates it: fused
    v = __builtin_fmaf(v_ne[c], ne, v);
    v = __builtin_fmaf(v_sw[c], sw, v);
    v = __builtin_fmaf(v_se[c], se, v);
    o[c] = v;
    sq += v * v;
  }
  sq = wave_sum(sq);
  const float nrm = fmaxf(sqrtf(sq), 1e-12f);  // F.normalize eps
#pragma unroll
  for (int c = 0; c < 4; ++c) o[c] = o[c] / nrm;
  return o;
}

// (the kernels below are written once as *_body<E>; the float32 kernels keep their names, the half ones are the *_typed_kernel<E>)
template <class E>
__device__ __forceinline__ void sample_desc_body(
    const float* __restrict__ pnt, const int* __restrict__ sub2line_g, const LinetrLineRec* __restrict__ recs,
    int64_t n_tokens, int T, const E* __restrict__ nhwc, int Hc, int Wc, int align_corners,
    float* __restrict__ desc) {
  const int64_t tok = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (tok >= n_tokens) return;
  const int lane = threadIdx.x & 63;
  const int n = (int)(tok / T);
  const int img = recs ? recs[sub2line_g[n]].image : 0;   // no records: all points belong to one image (linetr_sample_descriptors)
  const f32x4 o = sample_one(pnt[tok * 2 + 0], pnt[tok * 2 + 1], nhwc + (int64_t)img * Hc * Wc * D, Hc, Wc,
                             align_corners, lane);
  *reinterpret_cast<f32x4*>(desc + tok * D + lane * 4) = o;
}
static __global__ __launch_bounds__(256) void sample_desc_kernel(
    const float* __restrict__ pnt, const int* __restrict__ sub2line_g, const LinetrLineRec* __restrict__ recs,
    int64_t n_tokens, int T, const float* __restrict__ nhwc, int Hc, int Wc, int align_corners,
    float* __restrict__ desc) {
  sample_desc_body(pnt, sub2line_g, recs, n_tokens, T, nhwc, Hc, Wc, align_corners, desc);
}
template <class E>
static __global__ __launch_bounds__(256) void sample_desc_typed_kernel(
    const float* __restrict__ pnt, const int* __restrict__ sub2line_g, const LinetrLineRec* __restrict__ recs,
    int64_t n_tokens, int T, const E* __restrict__ nhwc, int Hc, int Wc, int align_corners,
    float* __restrict__ desc) {
  sample_desc_body(pnt, sub2line_g, recs, n_tokens, T, nhwc, Hc, Wc, align_corners, desc);
}

// ragged: map and size from the table entry of the token's image
template <class E>
__device__ __forceinline__ void sample_desc_ragged_body(
    const float* __restrict__ pnt, const int* __restrict__ sub2line_g, const LinetrLineRec* __restrict__ recs, int64_t n_tokens, int T,
    const RaggedImage* __restrict__ tab, int align_corners, float* __restrict__ desc) {
  const int64_t tok = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (tok >= n_tokens) return;
  const int lane = threadIdx.x & 63;
  const int n = (int)(tok / T);
  const int img = __builtin_amdgcn_readfirstlane(recs[sub2line_g[n]].image);   // one token per wave: its image is wave-uniform
  const f32x4 o = sample_one(pnt[tok * 2 + 0], pnt[tok * 2 + 1], (const E*)tab[img].nhwc, tab[img].Hc, tab[img].Wc, align_corners, lane);
  *reinterpret_cast<f32x4*>(desc + tok * D + lane * 4) = o;
}
static __global__ __launch_bounds__(256) void sample_desc_ragged_kernel(
    const float* __restrict__ pnt, const int* __restrict__ sub2line_g, const LinetrLineRec* __restrict__ recs, int64_t n_tokens, int T,
    const RaggedImage* __restrict__ tab, int align_corners, float* __restrict__ desc) {
  sample_desc_ragged_body<float>(pnt, sub2line_g, recs, n_tokens, T, tab, align_corners, desc);
}
template <class E>
static __global__ __launch_bounds__(256) void sample_desc_ragged_typed_kernel(
    const float* __restrict__ pnt, const int* __restrict__ sub2line_g, const LinetrLineRec* __restrict__ recs, int64_t n_tokens, int T,
    const RaggedImage* __restrict__ tab, int align_corners, float* __restrict__ desc) {
  sample_desc_ragged_body<E>(pnt, sub2line_g, recs, n_tokens, T, tab, align_corners, desc);
}

constexpr int KP_DESC_N = 64;     // key points per block
constexpr int KP_DESC_LS = KP_DESC_N + 1;
constexpr size_t KP_DESC_LDS = (size_t)D * KP_DESC_LS * 4;

// sample_descriptors (models/superpoint.py:81-93) for the packed key points of a batch: one block = up to 64 consecutive key points of ONE image, one wave per
// key point (sample_one), staged through LDS [256][65] so that the store along n is contiguous: image b owns [256][n_b] floats at
// out + 256 cu_kp[b].  grid ceil(n_total / 64) + B (an upper bound of the chunks; the block finds its image in cu_kp), block 256,
// dynamic LDS KP_DESC_LDS.
template <class E>
__device__ __forceinline__ void sp_kp_desc_body(const float* __restrict__ kp, const int* __restrict__ cu_kp, int B,
                                                const E* __restrict__ nhwc, int Hc, int Wc, int align_corners,
                                                float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float kp_tile[];
  int chunk = blockIdx.x, b = 0, start = 0, n_b = 0;
  for (; b < B; ++b) {
    start = cu_kp[b];
    n_b = cu_kp[b + 1] - start;
    const int nch = (n_b + KP_DESC_N - 1) / KP_DESC_N;
    if (chunk < nch) break;
    chunk -= nch;
  }
  if (b >= B) return;
  const int j0 = chunk * KP_DESC_N, nj = min(KP_DESC_N, n_b - j0);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const E* img = nhwc + (int64_t)b * Hc * Wc * D;
  for (int j = w; j < nj; j += 4) {
    const int64_t g = (int64_t)start + j0 + j;
    const f32x4 o = sample_one(kp[g * 2 + 0], kp[g * 2 + 1], img, Hc, Wc, align_corners, lane);
#pragma unroll
    for (int c = 0; c < 4; ++c) kp_tile[(lane * 4 + c) * KP_DESC_LS + j] = o[c];
  }
  __syncthreads();
  float* dst = out + (int64_t)D * start + j0;
  if (lane < nj)
    for (int ch = w * 64; ch < w * 64 + 64; ++ch) dst[(int64_t)ch * n_b + lane] = kp_tile[ch * KP_DESC_LS + lane];
}
static __global__ __launch_bounds__(256) void sp_kp_desc_kernel(const float* __restrict__ kp, const int* __restrict__ cu_kp, int B,
                                                         const float* __restrict__ nhwc, int Hc, int Wc, int align_corners,
                                                         float* __restrict__ out) {
  sp_kp_desc_body(kp, cu_kp, B, nhwc, Hc, Wc, align_corners, out);
}
template <class E>
static __global__ __launch_bounds__(256) void sp_kp_desc_typed_kernel(const float* __restrict__ kp, const int* __restrict__ cu_kp, int B,
                                                               const E* __restrict__ nhwc, int Hc, int Wc, int align_corners,
                                                               float* __restrict__ out) {
  sp_kp_desc_body(kp, cu_kp, B, nhwc, Hc, Wc, align_corners, out);
}

}  // namespace lt
