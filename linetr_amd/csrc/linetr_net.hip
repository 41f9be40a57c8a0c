// liblinetr_hip.so, translation unit 2 of 6: tokenise / forward / describe and the diagnostics entry points of the C ABI, the
// GEMM dispatcher, and every kernel of the descriptor network (csrc/lt_*.h).  The experiments build adds its paths through a
// few hooks, defined in experiments/csrc/lt_x_net.h, which this file includes behind sig_network.
#include <algorithm>
#include <array>
#include <numeric>
#include <set>

#include "lt_handle.h"
#include "lt_gemm.h"
#include "lt_gemm_split.h"
#include "lt_gemm_split16.h"
#include "lt_st_image.h"
#include "lt_gemm_small.h"
#include "lt_model.h"
#include "lt_attn.h"
#include "lt_attn_fused.h"
#include "lt_gemm_ws.h"
#include "lt_tokmlp.h"
#include "lt_token.h"
#include "lt_bntrain.h"

using namespace lt;

namespace {

// profile class of a GEMM launch, "<kind>_<tile>" (bench.py maps these names to kernel symbols), from a table made once.  tile:
// an F32Tile in the f32 mode (LINETR_PREC_F32 = 0), a SplitTile otherwise
const char* gemm_class_name(int precision, int tile, const GemmArgs& g, int groups) {
  static const auto names = [] {
    const char* kind[4] = {"gemm_f32", "gemm_bf16x3", "gemm_bf16x6", "gemm_f16x3"};   // by LINETR_PREC_*
    std::array<std::array<std::string, (int)SplitTile::count>, 4> n;
    for (int p = 0; p < 4; ++p)
      for (int t = 0; t < (p ? (int)SplitTile::count : (int)F32Tile::count); ++t)
        n[p][t] = std::string(kind[p]) + "_" + (p ? tile_name((SplitTile)t) : tile_name((F32Tile)t));
    return n;
  }();
  const std::string& name = names[precision][tile];
  // LINETR_PROFILE_SHAPES=1: one profile class per GEMM shape (tuning aid)
  static const bool by_shape = LT_XENV("LINETR_PROFILE_SHAPES") != nullptr;
  if (!by_shape) return name.c_str();
  static std::mutex mu;
  static std::set<std::string> shapes;
  char buf[160];
  snprintf(buf, sizeof buf, "%s[M=%d,N=%d,K=%d,g=%d]", name.c_str(), g.M, g.N, g.K, groups);
  std::lock_guard<std::mutex> lock(mu);
  return shapes.insert(buf).first->c_str();
}

// Operands of run_gemm, row-major with row strides in floats.  A: the left operand; with p2 its columns K1.. come from a second
// matrix ([A | A2]).  Y: the output.
struct GemmA { const float* p; int ld; const float* p2 = nullptr; int ld2 = 0, K1 = 0; };
struct GemmY { float* p; int ld; };
// n independent products over consecutive N-row blocks of the weight (and of its bias); group i reads A + i gA, writes Y + i gY
struct GemmGroups { int n, N; int64_t gA, gY; };

struct NormSpec {          // row normalisation that follows a [M,256] GEMM (see GemmArgs::norm)
  int mode = 0;            // 1 LayerNorm, 2 L2
  const float* gamma = nullptr;
  const float* beta = nullptr;
  const float* add2 = nullptr;   // added after the normalisation, row stride 256
  float eps = 0.f;
};

// the experiments build's hooks (experiments/csrc/lt_x_net.h)
#ifdef LINETR_EXPERIMENTS
int x_gemm(LinetrHandle*, hipStream_t, SplitGemmArgs& sa, const GemmW& w, int groups, const NormSpec*, double fl, double by, bool& done);
int x_split_weights(LinetrHandle* H, std::vector<GemmWSpec>& weights);
int64_t x_ws_bytes(const LinetrHandle* h, int N);
#endif

// the kernels' arguments of Y = norm(act(A W^T + b) (+ R)), R with Y's row stride; fails on a shape the weight w does not have
int gemm_args(const GemmW& w, int M, const GemmA& A, const GemmY& Y, int act, const float* R, const GemmGroups* grp,
              const NormSpec* ns, GemmArgs& g) {
  const int groups = grp ? grp->n : 1, N = grp ? grp->N : w.rows;
  if (A.p2 && (A.K1 <= 0 || A.K1 >= w.K)) return fail(LINETR_E_ARG, "gemm: split point K1 = %d outside (0, K = %d)", A.K1, w.K);
  if ((int64_t)N * groups > w.rows) return fail(LINETR_E_ARG, "gemm: %d groups of %d rows exceed the weight's %d", groups, N, w.rows);
  // the kernels step A, W, the bias and Y from group to group, nothing else
  if (groups > 1 && (R || ns)) return fail(LINETR_E_ARG, "gemm: a grouped launch takes no residual and no row normalisation");
  g = GemmArgs{};
  g.A = A.p; g.lda = A.ld; g.A2 = A.p2; g.lda2 = A.ld2; g.K1 = A.K1;
  g.W = w.W; g.ldw = w.K; g.bias = w.b; g.R = R; g.ldr = Y.ld; g.Y = Y.p; g.ldy = Y.ld;
  g.M = M; g.N = N; g.K = w.K; g.act = act;
  if (grp) { g.gA = grp->gA; g.gW = (int64_t)N * w.K; g.gBias = N; g.gY = grp->gY; }
  if (ns) { g.norm = ns->mode; g.gamma = ns->gamma; g.beta = ns->beta; g.add2 = ns->add2; g.ldadd2 = D; g.eps = ns->eps; }
  return LINETR_OK;
}

// every token row of the batch through a K = 128 layer: weights stay in registers, rows stream (lt_gemm_ws.h).  What the kernel
// can run (gemm_ws_able) and what the dispatcher gives it (gemm_ws_takes: token-count sizes)
bool gemm_ws_able(const LinetrHandle* h, const GemmArgs& g, const GemmW& w, int groups, const NormSpec* fused_norm) {
  return h->precision == LINETR_PREC_BF16X6 && groups == 1 && !g.A2 && !g.R && !fused_norm && w.st &&
         gemm_ws_can(g.N, g.K, g.lda, g.ldy, g.act);
}
bool gemm_ws_takes(const LinetrHandle* h, const GemmArgs& g, const GemmW& w, int groups, const NormSpec* fused_norm) {
  return gemm_ws_able(h, g, w, groups, fused_norm) && gemm_ws_fits(g.M, g.N, g.K, g.lda, g.ldy, g.act) && !LT_XENV("LINETR_NO_GEMM_WS");
}

// One kernel of the family chosen by hand (linetr_debug_gemm_case): `tile` -1 = the dispatcher's choice, LINETR_GEMM_TILE_WS = the
// weight-stationary kernel, otherwise an F32Tile (f32 mode) / SplitTile index.  `used` receives what launches, after the
// launchers' fallback rules; launch = false only reports it.
struct GemmForce { int tile = -1; int* used = nullptr; bool launch = true; };

int run_gemm(LinetrHandle* h, hipStream_t st, const GemmW& w, int M, const GemmA& A, const GemmY& Y, int act, const float* R = nullptr,
             const GemmGroups* grp = nullptr, const NormSpec* fused_norm = nullptr, const GemmForce* force = nullptr) {
  GemmArgs g;
  if (int e = gemm_args(w, M, A, Y, act, R, grp, fused_norm, g)) return e;
  const int groups = grp ? grp->n : 1;
  const int forced = force ? force->tile : -1;
  const bool launch = !force || force->launch;
  auto report = [&](int tile) { if (force && force->used) *force->used = tile; };
  const double fl = 2.0 * M * (double)g.N * g.K * groups;
  const double by = 4.0 * groups * ((double)M * g.K + (double)g.N * g.K + (double)M * g.N);
  if (h->precision == LINETR_PREC_F32) {
    if (forced >= (int)F32Tile::count) return fail(LINETR_E_ARG, "gemm: the f32 mode has no tile %d", forced);
    if (fused_norm) return fail(LINETR_E_ARG, "gemm: the f32 kernels have no fused row normalisation");
    const F32Tile tile = f32_tile_launched(g, forced < 0 ? f32_tile(g, groups) : (F32Tile)forced);
    report((int)tile);
    if (!launch) return LINETR_OK;
    ProfScope ps(h, st, gemm_class_name(LINETR_PREC_F32, (int)tile, g, groups), fl, by);
    return gemm_launch(g, groups, tile, st);
  }
  SplitGemmArgs sa;
  sa.g = g;
#ifdef LINETR_EXPERIMENTS
  if (!force) {
    bool done = false;   // done: the stream-K or the row-owner GEMM took the launch
    if (int e = x_gemm(h, st, sa, w, groups, fused_norm, fl, by, done); e || done) return e;
  }
#endif
  if (forced == LINETR_GEMM_TILE_WS && !gemm_ws_able(h, g, w, groups, fused_norm))
    return fail(LINETR_E_ARG, "gemm: the weight-stationary kernel runs act(A[M,128] W[256,128]^T + b) in bf16x6 only, act none / ReLU");
  if (forced == LINETR_GEMM_TILE_WS || (forced < 0 && gemm_ws_takes(h, g, w, groups, fused_norm))) {
    report(LINETR_GEMM_TILE_WS);
    if (!launch) return LINETR_OK;
    WsGemmArgs a;
    a.A = A.p; a.lda = A.ld; a.Wst = w.st; a.bias = w.b ? w.b : h->zeros; a.Y = Y.p; a.ldy = Y.ld; a.M = M; a.act = act;
    ProfScope ps(h, st, "gemm_bf16x6_ws64x256", fl, by);
    return gemm_ws_launch(a, st);
  }
  const int pl = h->precision == LINETR_PREC_BF16X6 ? 3 : 2;
  SplitTile tile;
  if (forced >= (int)SplitTile::count) return fail(LINETR_E_ARG, "gemm: no split tile %d", forced);
  if (forced >= 0) tile = (SplitTile)forced;
  else if (int e = pick_split_tile(g, groups, pl, tile)) return e;
  if (int e = split_tile_launched(g, groups, pl, tile)) return e;
  report((int)tile);
  if (!launch) return LINETR_OK;
  ProfScope ps(h, st, gemm_class_name(h->precision, (int)tile, g, groups), fl, by);
  switch (h->precision) {
    case LINETR_PREC_BF16X3: sa.Wsp = w.s2; sa.gWsp = g.gW * 4; return gemm_split_launch<2>(sa, groups, tile, st);
    case LINETR_PREC_F16X3: sa.Wsp = w.h2; sa.gWsp = g.gW * 4; return gemm_split_launch<2, 1>(sa, groups, tile, st);
    default: sa.Wsp = w.s3; sa.gWsp = g.gW * 6; return gemm_split_launch<3>(sa, groups, tile, st);
  }
}

// does the dispatcher's tile for this [M,256] product normalise the rows in its epilogue?
bool gemm_norm_fuses(const LinetrHandle* h, const GemmW& w, int M, const GemmA& A, const float* R, float* Y) {
  GemmArgs g;   // (LINETR_NO_FUSED_NORM: a tuning / test aid, read per call)
  return !LT_XENV("LINETR_NO_FUSED_NORM") && h->precision != LINETR_PREC_F32 && !LT_XENV("LINETR_GEMM_TILE") &&
         !gemm_args(w, M, A, {Y, D}, ACT_NONE, R, nullptr, nullptr, g) &&
         split_tile(g, 1, h->precision == LINETR_PREC_BF16X6 ? 3 : 2) == SplitTile::t128x256;
}

int row_norm(LinetrHandle* h, hipStream_t st, const float* x, int M, const NormSpec& ns, float* Y) {
  ProfScope ps(h, st, "row_norm", 0, (double)M * D * (ns.add2 ? 12 : 8));
  hipLaunchKernelGGL(row_norm_kernel, dim3(cdiv(M, 4)), dim3(256), 0, st, x, M, ns.mode == 2 ? 1 : 0, ns.gamma, ns.beta,
                     ns.add2, ns.eps, Y);
  LT_LAUNCH_CHECK();
  return 0;
}

// Y[M,256] = norm(epi(A W^T + bias) (+ R)) (+ add2), R and Y with row stride 256.  The split-bf16 128x256 tile owns complete rows
// and normalises them in its epilogue (one launch and one [M,256] round trip less); every other case runs the GEMM into `tmp` and
// then row_norm_kernel.  Same arithmetic either way.
int run_gemm_norm(LinetrHandle* h, hipStream_t st, const GemmW& w, int M, const GemmA& A, const float* R, float* tmp, float* Y,
                  const NormSpec& ns) {
  if (w.rows != D) return fail(LINETR_E_ARG, "gemm_norm: the weight has %d rows, not %d", w.rows, D);
  if (gemm_norm_fuses(h, w, M, A, R, Y)) return run_gemm(h, st, w, M, A, {Y, D}, ACT_NONE, R, nullptr, &ns);
  if (int e = run_gemm(h, st, w, M, A, {tmp, D}, ACT_NONE, R)) return e;
  return row_norm(h, st, tmp, M, ns, Y);
}

// Where one weight's split copies go in a buffer, from byte `off` on (advanced past them): the three split planes, then (with_st)
// the split-tile image on a 1024-byte boundary.  The handle's arena and linetr_debug_gemm's scratch buffers are laid out this way.
struct SplitOffsets { int64_t s2, s3, h2, st = -1; };
SplitOffsets split_offsets(int64_t rows, int K, bool with_st, int64_t& off) {
  SplitOffsets o;
  o.s2 = off; off += align_up(rows * K * 4, 256);
  o.s3 = off; off += align_up(rows * K * 6, 256);
  o.h2 = off; off += align_up(rows * K * 4, 256);
  if (with_st) { off = align_up(off, 1024); o.st = off; off += st_bytes(rows, K); }   // ST image (rows padded to 128)
  return o;
}

// points w at its split copies at base + o, and (make) makes them from w.W on stream st
void split_copies(GemmW& w, unsigned char* base, const SplitOffsets& o, bool make, hipStream_t st) {
  w.s2 = base + o.s2; w.s3 = base + o.s3; w.h2 = base + o.h2;
  w.st = o.st >= 0 ? base + o.st : nullptr;
  if (!make) return;
  const dim3 grid((unsigned)cdiv((int)((int64_t)w.rows * w.K / 4), 256));
  hipLaunchKernelGGL(split_rows_kernel<2>, grid, dim3(256), 0, st, w.W, base + o.s2, (int64_t)w.rows, w.K);
  hipLaunchKernelGGL(split_rows_kernel<3>, grid, dim3(256), 0, st, w.W, base + o.s3, (int64_t)w.rows, w.K);
  hipLaunchKernelGGL((split_rows_kernel<2, 1>), grid, dim3(256), 0, st, w.W, base + o.h2, (int64_t)w.rows, w.K);
  if (o.st >= 0) {
    const int64_t thr = st_row_blocks(w.rows) * (w.K / 16) * 32;
    hipLaunchKernelGGL(to_st_kernel, dim3((unsigned)((thr + 255) / 256)), dim3(256), 0, st, w.W, w.K, w.rows, w.K / 16, base + o.st);
  }
}

}  // namespace

// split-bf16 / fp16 / split-tile copies of the prepared GEMM weights (called once by linetr_create)
int lt::make_split_copies(LinetrHandle* H, std::vector<GemmWSpec> weights) {
#ifdef LINETR_EXPERIMENTS
  if (int e = x_split_weights(H, weights)) return e;
#endif
  int64_t total = 0;
  std::vector<SplitOffsets> at;
  // the weights that travel by LDS-DMA or stay in registers / LDS get an ST image
  for (auto& s : weights) at.push_back(split_offsets(s.w->rows, s.w->K, s.st && s.w->rows % 16 == 0 && s.w->K % 32 == 0, total));
  LT_HIP(hipMalloc((void**)&H->split_arena, total));
  LT_HIP(hipMalloc((void**)&H->zeros, 4096 * sizeof(float)));
  LT_HIP(hipMemset(H->zeros, 0, 4096 * sizeof(float)));
  for (size_t i = 0; i < weights.size(); ++i) split_copies(*weights[i].w, H->split_arena, at[i], true, 0);
  LT_LAUNCH_CHECK();
  LT_HIP(hipDeviceSynchronize());
  return LINETR_OK;
}

// =============================================================================================
// tokenise
// =============================================================================================

namespace {
// where each image's mat_klines2sublines block goes (LinetrTokens.mat); cu_sub may be NULL for a single image
int k2s_table(const LinetrTokens& out, int n_images, int K, int N, const int32_t* h_cu_sub, K2sTable& tab, const char* who) {
  tab = K2sTable{};
  if (!out.mat) return 0;
  if (n_images > K2S_MAX_IMAGES) return fail(LINETR_E_ARG, "%s: mat_klines2sublines is written for calls of up to %d images", who, K2S_MAX_IMAGES);
  if (n_images == 1) {   // whatever image index the caller's records carry, it is this one image
    for (int i = 0; i < K2S_MAX_IMAGES; ++i) tab.img[i] = K2sImage{0, N, 0};
    return 0;
  }
  if (!out.h_cu_klines || !h_cu_sub) return fail(LINETR_E_ARG, "%s: mat_klines2sublines of several images needs the host prefix sums of key-lines and sub-lines", who);
  if (out.h_cu_klines[n_images] != K) return fail(LINETR_E_ARG, "%s: h_cu_klines does not end at K", who);
  int64_t off = 0;
  for (int i = 0; i < n_images; ++i) {
    const int ki = out.h_cu_klines[i + 1] - out.h_cu_klines[i], ni = h_cu_sub[i + 1] - h_cu_sub[i];
    if (ki < 0 || ni < 0) return fail(LINETR_E_ARG, "%s: prefix sums not monotone", who);
    tab.img[i] = K2sImage{off, ni, h_cu_sub[i]};
    off += (int64_t)ki * ni;
  }
  return 0;
}

// The channel-last form of n_images dense descriptor maps of P positions: the map itself when it is NHWC already (the repo's producer:
// read in place), otherwise its transpose, made in `buf`
// One launch for whatever the map's element type is: the float32 kernel KF32, or the half kernel KTYPED, an expression in E (f16_t or
// bf16_t) in parentheses.  The arguments may use E as well: `(const E*)map`.
#define LT_LAUNCH_BY_ELEM(type, KF32, KTYPED, grid, block, lds, st, ...)                                             \
  do {                                                                                                               \
    if ((type) == MT_F32) { typedef float E; (void)sizeof(E); hipLaunchKernelGGL(KF32, grid, block, lds, st, __VA_ARGS__); }       \
    else if ((type) == MT_F16) { typedef f16_t E; (void)sizeof(E); hipLaunchKernelGGL(KTYPED, grid, block, lds, st, __VA_ARGS__); } \
    else { typedef bf16_t E; (void)sizeof(E); hipLaunchKernelGGL(KTYPED, grid, block, lds, st, __VA_ARGS__); }                      \
  } while (0)

int nhwc_map(LinetrHandle* h, hipStream_t st, const void* dense_desc, const MapFormat& mf, int n_images, int P, void* buf,
             const void*& nhwc) {
  nhwc = dense_desc;
  if (mf.nhwc) return LINETR_OK;
  ProfScope ps(h, st, "nchw_to_nhwc", 0, 2.0 * n_images * P * D * mf.esize);
  if (mf.type == MT_F32)
    hipLaunchKernelGGL(nchw_to_nhwc_kernel, dim3(cdiv(P, 64), D / 64, n_images), dim3(256), 0, st, (const float*)dense_desc, (float*)buf, D, P);
  else   // halves move as they are: one kernel for both half types
    hipLaunchKernelGGL(nchw_to_nhwc_half_kernel, dim3(cdiv(P, 64), D / 64, n_images), dim3(256), 0, st, (const uint16_t*)dense_desc,
                       (uint16_t*)buf, D, P);
  LT_LAUNCH_CHECK();
  nhwc = buf;
  return LINETR_OK;
}

// The token front end of linetr_tokenize and linetr_describe: line_fill -> tokenize -> layout pass -> (out.desc) sample_desc.
struct TokenFront {
  const LinetrLineRec* recs; int K, N; double td; int T;
  const void* dense_desc; const float* dense_score;
  int n_images, height, width, align_corners; MapFormat mf;   // mf: layout and element type of dense_desc (one for all images)
  double clip_x, clip_y;               // end points are clipped to the caller's clip size (tokenize) or the map's own (describe)
  float *sublines, *resp, *angle_sub;  // the caller's tensors, or workspace where it asked for none
  int* s2l_g;                          // workspace: sub-line -> key-line of the batch
  void* nhwc_buf;                      // workspace: the transposed map (in the map's element type)
  bool map_always;                     // the layout pass runs without out.desc too (describe: the pooling kernel reads the map)
  double tokenize_bytes;               // what the `tokenize` profile class is charged
  // describe only: the compact list of real tokens, closed by one padding row per image (written by cdiv(n_pad_images, 64) more blocks)
  float *cpnt = nullptr, *cscore = nullptr; int n_pad_images = 0; int64_t first_pad = 0;
  // ragged (linetr_describe_ragged): the image table in the workspace; the kernels take size, token distance, clip and maps from it and
  // the nine uniform fields above are unused.  max_cells = the largest image's Hc * Wc, cells = their sum (the layout pass)
  const RaggedImage* tab = nullptr; int max_cells = 0; double cells = 0;
};
int token_front(LinetrHandle* h, hipStream_t st, const TokenFront& a, const LinetrTokens& out, const K2sTable& k2s, int32_t* d_sub2line,
                const void*& nhwc) {
  {
    ProfScope ps(h, st, "line_fill", 0, (double)a.K * 80 + (double)a.N * 8);
    if (a.tab)
      hipLaunchKernelGGL(line_fill_ragged_kernel, dim3(cdiv(a.K, 256)), dim3(256), 0, st, a.recs, a.K, a.tab, out.klines, out.length,
                         out.angles, a.s2l_g, d_sub2line);
    else
      hipLaunchKernelGGL(line_fill_kernel, dim3(cdiv(a.K, 256)), dim3(256), 0, st, a.recs, a.K, a.clip_x, a.clip_y, out.klines, out.length,
                         out.angles, a.s2l_g, d_sub2line);
    LT_LAUNCH_CHECK();
  }
  {
    ProfScope ps(h, st, "tokenize", 0, a.tokenize_bytes);
    // (with out.mat: K more blocks write the rows of mat_klines2sublines in the same launch)
    const dim3 grid(a.N + cdiv(a.n_pad_images, 64) + (out.mat ? a.K : 0));
    if (a.tab)
      hipLaunchKernelGGL(tokenize_ragged_kernel, grid, dim3(64), 0, st, a.recs, a.s2l_g, a.N, a.T, a.tab, a.sublines, out.pnt, out.mask,
                         a.resp, a.angle_sub, out.score, a.cpnt, a.cscore, a.n_pad_images, a.first_pad, out.mat, k2s);
    else
      hipLaunchKernelGGL(tokenize_kernel, grid, dim3(64), 0, st, a.recs, a.s2l_g, a.N,
                         a.td, a.T, a.height, a.width, a.clip_x, a.clip_y, a.dense_score, a.sublines, out.pnt, out.mask, a.resp, a.angle_sub,
                         out.score, a.cpnt, a.cscore, a.n_pad_images, a.first_pad, out.mat, k2s);
    LT_LAUNCH_CHECK();
  }
  const int64_t ntok = (int64_t)a.N * a.T;
  nhwc = nullptr;
  if (a.tab) {   // every image's channel-last map is where its table entry says: the caller's own, or the copy this pass makes
    if (!a.mf.nhwc) {
      ProfScope ps(h, st, "nchw_to_nhwc", 0, 2.0 * a.cells * D * a.mf.esize);
      if (a.mf.type == MT_F32)
        hipLaunchKernelGGL(nchw_to_nhwc_ragged_kernel, dim3(cdiv(a.max_cells, 64), D / 64, a.n_images), dim3(256), 0, st, a.tab, D);
      else
        hipLaunchKernelGGL(nchw_to_nhwc_half_ragged_kernel, dim3(cdiv(a.max_cells, 64), D / 64, a.n_images), dim3(256), 0, st, a.tab, D);
      LT_LAUNCH_CHECK();
    }
    if (out.desc) {
      ProfScope ps(h, st, "sample_desc", 0, (double)ntok * D * 4 * 2);
      LT_LAUNCH_BY_ELEM(a.mf.type, sample_desc_ragged_kernel, (sample_desc_ragged_typed_kernel<E>), dim3((unsigned)((ntok + 3) / 4)),
                        dim3(256), 0, st, out.pnt, a.s2l_g, a.recs, ntok, a.T, a.tab, a.align_corners, out.desc);
      LT_LAUNCH_CHECK();
    }
    return LINETR_OK;
  }
  const int Hc = a.height / 8, Wc = a.width / 8;
  if (a.map_always || out.desc)
    if (int e = nhwc_map(h, st, a.dense_desc, a.mf, a.n_images, Hc * Wc, a.nhwc_buf, nhwc)) return e;
  if (out.desc) {   // the reference's dense [N, T, 256] tensor
    ProfScope ps(h, st, "sample_desc", 0, (double)ntok * D * 4 * 2);
    LT_LAUNCH_BY_ELEM(a.mf.type, sample_desc_kernel, (sample_desc_typed_kernel<E>), dim3((unsigned)((ntok + 3) / 4)), dim3(256), 0, st,
                      out.pnt, a.s2l_g, a.recs, ntok, a.T, (const E*)nhwc, Hc, Wc, a.align_corners, out.desc);
    LT_LAUNCH_CHECK();
  }
  return LINETR_OK;
}

// workspace of linetr_tokenize: channel-last copy of an NCHW descriptor map | global sub-line -> key-line map
struct TokLayout { int64_t o_nhwc, o_s2l, total; };
TokLayout tok_layout(int n_images, int height, int width, int N) {
  TokLayout L{};
  Carve c;
  L.o_nhwc = c.take(sz_mul(n_images, height / 8, width / 8, D * 4));
  L.o_s2l = c.take((int64_t)std::max(N, 1) * 4);
  L.total = sz_add(c.o, 256);
  return L;
}
}  // namespace

extern "C" int64_t linetr_tokenize_workspace_bytes(int32_t n_images, int32_t height, int32_t width, int32_t N) {
  return sz_answer(tok_layout(n_images, height, width, N).total);
}

extern "C" int linetr_tokenize(LinetrHandle* h, const LinetrLineRec* d_recs, int32_t K, int32_t N, double td,
                               int32_t T, const void* d_dense_desc, const float* d_dense_score, int32_t n_images,
                               int32_t height, int32_t width, int32_t clip_height, int32_t clip_width, int32_t align_corners,
                               int32_t dense_is_nhwc, LinetrTokens out, int32_t* d_sub2line, void* d_ws, int64_t ws_bytes,
                               void* stream) {
  if (K <= 0 || N <= 0) return LINETR_OK;
  if (clip_height <= 0) clip_height = height;
  if (clip_width <= 0) clip_width = width;
  if (!d_recs || !d_dense_score || !out.sublines || !out.pnt || !out.mask || !out.resp || !out.angle_sub ||
      !out.score || (out.desc && !d_dense_desc))
    return fail(LINETR_E_ARG, "tokenize: null pointer");
  if (T < 1 || T > 4096 || height % 8 || width % 8) return fail(LINETR_E_ARG, "tokenize: bad max_tokens / image size");
  MapFormat mf;
  if (int e = map_format(dense_is_nhwc, "tokenize", mf)) return e;
  if (!mf.aligned(d_dense_desc) || !aligned16(out.desc) || !aligned16(d_ws))
    return fail(LINETR_E_ARG, "tokenize: a channel-last descriptor map, out.desc and the workspace must be 16-byte aligned (a half channel-last map: 8-byte)");
  if (out.mat && n_images != 1) return fail(LINETR_E_ARG, "tokenize: mat_klines2sublines of several images: use linetr_describe (it has the sub-line prefix sums)");
  K2sTable k2s;
  if (int e = k2s_table(out, n_images, K, N, nullptr, k2s, "tokenize")) return e;
  const TokLayout L = tok_layout(n_images, height, width, N);
  if (ws_bytes < L.total) return fail(LINETR_E_WORKSPACE, "tokenize: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  if (h) LT_HIP(hipSetDevice(h->device));   // no weights involved: without a handle the current device is used
  TokenFront f{d_recs, K, N, td, T, d_dense_desc, d_dense_score, n_images, height, width, align_corners, mf,
               (double)clip_width - 0.6, (double)clip_height - 0.6, out.sublines, out.resp, out.angle_sub};
  f.nhwc_buf = (char*)d_ws + L.o_nhwc;
  f.s2l_g = (int*)((char*)d_ws + L.o_s2l);
  f.map_always = false;
  f.tokenize_bytes = (double)N * T * 16;
  const void* nhwc;
  return token_front(h, st, f, out, k2s, d_sub2line, nhwc);
}

// sample_descriptors (models/line_process.py:86-98) on its own: n points of ONE image
// (a format the calls refuse: SZ_LIMIT, which the queries answer with 0 and no workspace satisfies)
static int64_t nhwc_copy_bytes(int B, int Hc, int Wc, int dense_is_nhwc) {
  MapFormat mf;
  if (!map_format_ok(dense_is_nhwc, mf)) return SZ_LIMIT;
  return mf.nhwc ? 0 : align_up(sz_mul(B, Hc, Wc, D * mf.esize), 256);
}
extern "C" int64_t linetr_sample_descriptors_workspace_bytes(int32_t Hc, int32_t Wc, int32_t dense_is_nhwc) {
  return sz_answer(nhwc_copy_bytes(1, Hc, Wc, dense_is_nhwc));
}

extern "C" int linetr_sample_descriptors(LinetrHandle* h, const float* d_points, int64_t n, const void* d_dense_desc, int32_t Hc,
                                         int32_t Wc, int32_t align_corners, int32_t dense_is_nhwc, float* d_out, void* d_ws,
                                         int64_t ws_bytes, void* stream) {
  if (n < 0 || Hc <= 0 || Wc <= 0) return fail(LINETR_E_ARG, "sample_descriptors: bad shape");
  if (n == 0) return LINETR_OK;
  if (!d_points || !d_dense_desc || !d_out) return fail(LINETR_E_ARG, "sample_descriptors: null pointer");
  MapFormat mf;
  if (int e = map_format(dense_is_nhwc, "sample_descriptors", mf)) return e;
  if (!mf.aligned(d_dense_desc) || !aligned16(d_out) || !aligned16(d_ws))
    return fail(LINETR_E_ARG, "sample_descriptors: a channel-last descriptor map, the output and the workspace must be 16-byte aligned (a half channel-last map: 8-byte)");
  if (ws_bytes < nhwc_copy_bytes(1, Hc, Wc, dense_is_nhwc) || (!mf.nhwc && !d_ws))
    return fail(LINETR_E_WORKSPACE, "sample_descriptors: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  if (h) LT_HIP(hipSetDevice(h->device));
  const void* nhwc;
  if (int e = nhwc_map(h, st, d_dense_desc, mf, 1, Hc * Wc, d_ws, nhwc)) return e;
  ProfScope ps(h, st, "sample_desc", 0, (double)n * D * 4 * 2);
  // T = 1 and no records: every point is its own "sub-line" of image 0
  LT_LAUNCH_BY_ELEM(mf.type, sample_desc_kernel, (sample_desc_typed_kernel<E>), dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, d_points,
                    (const int*)nullptr, (const LinetrLineRec*)nullptr, n, 1, (const E*)nhwc, Hc, Wc, align_corners, d_out);
  LT_LAUNCH_CHECK();
  return LINETR_OK;
}

// sample_descriptors (models/superpoint.py:81-93) for the packed key points of a batch (the output of linetr_superpoint_keypoints)
extern "C" int64_t linetr_point_descriptors_workspace_bytes(int32_t B, int32_t Hc, int32_t Wc, int32_t dense_is_nhwc) {
  return sz_answer(nhwc_copy_bytes(std::max(B, 0), std::max(Hc, 0), std::max(Wc, 0), dense_is_nhwc));
}

extern "C" int linetr_point_descriptors(LinetrHandle* h, const float* d_keypoints, const int32_t* d_cu_kp, int32_t B, int64_t n_total,
                                        const void* d_dense_desc, int32_t Hc, int32_t Wc, int32_t align_corners, int32_t dense_is_nhwc,
                                        float* d_desc_cn, void* d_ws, int64_t ws_bytes, void* stream) {
  if (B < 0 || n_total < 0 || Hc <= 0 || Wc <= 0 || n_total > INT32_MAX) return fail(LINETR_E_ARG, "point_descriptors: bad shape");
  if (B == 0 || n_total == 0) return LINETR_OK;
  if (!d_keypoints || !d_cu_kp || !d_dense_desc || !d_desc_cn) return fail(LINETR_E_ARG, "point_descriptors: null pointer");
  MapFormat mf;
  if (int e = map_format(dense_is_nhwc, "point_descriptors", mf)) return e;
  if (!mf.aligned(d_dense_desc) || !aligned16(d_ws))
    return fail(LINETR_E_ARG, "point_descriptors: a channel-last descriptor map and the workspace must be 16-byte aligned (a half channel-last map: 8-byte)");
  if (ws_bytes < nhwc_copy_bytes(B, Hc, Wc, dense_is_nhwc) || (!mf.nhwc && !d_ws))
    return fail(LINETR_E_WORKSPACE, "point_descriptors: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  if (h) LT_HIP(hipSetDevice(h->device));
  if (mf.type == MT_F32) LT_HIP(allow_dynamic_lds<sp_kp_desc_kernel>((int)KP_DESC_LDS));   // 65 KiB
  else if (mf.type == MT_F16) LT_HIP(allow_dynamic_lds<sp_kp_desc_typed_kernel<f16_t>>((int)KP_DESC_LDS));
  else LT_HIP(allow_dynamic_lds<sp_kp_desc_typed_kernel<bf16_t>>((int)KP_DESC_LDS));
  const void* nhwc;
  if (int e = nhwc_map(h, st, d_dense_desc, mf, B, Hc * Wc, d_ws, nhwc)) return e;
  ProfScope ps(h, st, "sp_kp_desc", 0, (double)n_total * D * 4 * 5);
  LT_LAUNCH_BY_ELEM(mf.type, sp_kp_desc_kernel, (sp_kp_desc_typed_kernel<E>), dim3((unsigned)((n_total + KP_DESC_N - 1) / KP_DESC_N + B)),
                    dim3(256), KP_DESC_LDS, st, d_keypoints, d_cu_kp, B, (const E*)nhwc, Hc, Wc, align_corners, d_desc_cn);
  LT_LAUNCH_CHECK();
  return LINETR_OK;
}

// =============================================================================================
// forward
// =============================================================================================

namespace {
// W2 + residual + next q/k/v projection as one contraction (SigLayer::Wnext) is taken up to this many sub-lines: the sizes at which
// its N = 1024, K = 768 product still goes to the latency kernel (small_gemm_wins) -- above, 2.4x the flops cost more than a launch
constexpr int SIG_FOLD_MAX_ROWS = 960;
struct FwdWs {
  float* act[2][4];                                // the positional encoders' activations, layers 1-4: ENC_WORD [rows, .], ENC_LINE [N, .]
  float *pooled, *att, *fc, *o, *f1, *f2, *lpos, *zA, *zB, *qkv, *msgp, *msg, *hid;
  float *zqA, *zqB;                                // [N][4D] = [x_out | q/k/v of the next layer] (single-pair sizes: SigLayer::Wnext)
  int* cu;
  float* tap = nullptr;                            // linetr_debug_stage only: [L-1][N][D], x_out behind signature layers 0 .. L-2
  char* x = nullptr;                               // experiments build: where its own buffers start (lt_x_net.h)
  int64_t total;
};
FwdWs fwd_layout(const LinetrHandle* h, int N, int64_t rows, int n_images, char* base) {
  const LinetrModelConfig& c = h->cfg;
  FwdWs w;
  int64_t off = 0;
  auto take = [&](int64_t floats) { float* p = (float*)(base + off); off += align_up(floats * 4, 256); return p; };
  for (int i = 0; i < 4; ++i) w.act[ENC_WORD][i] = take(rows * c.enc_channels[i]);
  w.pooled = take((int64_t)N * HEADS * POOLW);
  w.att = take((int64_t)N * D); w.fc = take((int64_t)N * D); w.o = take((int64_t)N * D);
  w.f1 = take((int64_t)N * c.d_inner); w.f2 = take((int64_t)N * D);
  for (int i = 0; i < 4; ++i) w.act[ENC_LINE][i] = take((int64_t)N * c.enc_channels[i]);
  w.lpos = take((int64_t)N * D);
  w.zA = take((int64_t)N * D); w.zB = take((int64_t)N * D);
  w.qkv = take((int64_t)N * 3 * D); w.msgp = take((int64_t)N * D); w.msg = take((int64_t)N * D);
  w.hid = take((int64_t)N * 2 * D);
  const int64_t nq = N <= SIG_FOLD_MAX_ROWS ? (int64_t)N * 4 * D : 0;
  w.zqA = take(nq); w.zqB = take(nq);
  w.cu = (int*)take(n_images + 1);
#ifdef LINETR_EXPERIMENTS
  w.x = base + off; off += x_ws_bytes(h, N);
#endif
  w.total = off;
  return w;
}
}  // namespace

extern "C" int64_t linetr_forward_workspace_bytes(const LinetrHandle* h, int32_t N, int32_t T) {
  if (!h) return -1;
  // the image count only sizes a tiny prefix-sum array; reserve for the worst case (every sub-line its own image)
  return fwd_layout(h, std::max(N, 1), (int64_t)std::max(N, 1) * T, std::max(N, 1), nullptr).total;
}

namespace {
// Cut points of a pipelined batch (linetr_describe_submit), in launch order.  Stage k = the launches between cut k - 1 and cut k, on
// stream k of the handle's pipeline; the next stage's stream waits for an event recorded at the cut.
enum {
  CUT_TOKENS = 0,     // behind the tokeniser and the layout pass
  CUT_MLP = 1,        // behind the positional encoders' MLPs
  CUT_POOL = 2,       // behind the CLS pooling + value projection
  CUT_SENTENCE = 3,   // behind the descriptive layer's tail: in front of the line-signature network
  CUT_SIG0 = 4        // CUT_SIG0 + l: behind signature layer l
};
struct PipeStages {
  hipStream_t stream[LinetrHandle::PIPE_STREAMS];
  hipEvent_t ev[LinetrHandle::PIPE_STREAMS - 1];
  int cut[LinetrHandle::PIPE_STREAMS - 1];
  int n_cuts = 0, next = 0;
};
// at position `pos` of the launch sequence: if the plan cuts here, everything that follows is queued on the next stage's stream
int pipe_boundary(PipeStages* p, int pos, hipStream_t& st) {
  if (!p || p->next >= p->n_cuts || p->cut[p->next] != pos) return LINETR_OK;
  LT_HIP(hipEventRecord(p->ev[p->next], st));
  LT_HIP(hipStreamWaitEvent(p->stream[p->next + 1], p->ev[p->next], 0));
  st = p->stream[++p->next];
  return LINETR_OK;
}

struct TokenStage {            // how the token stage (word MLP + CLS pooling) is fed
  // dense path (linetr_forward): [N,T] tensors of the reference
  const float *pnt = nullptr, *score = nullptr, *desc = nullptr;
  // fused path (linetr_describe): compact real-token list + NHWC map
  const float *cpnt = nullptr, *cscore = nullptr; const void* nhwc = nullptr; int map_type = MT_F32;   // (the map's element type)
  const LinetrLineRec* recs = nullptr;
  const int* sub2line_g = nullptr;
  int64_t rows = 0;            // rows of the word-MLP GEMMs (N*T dense, n_real + n_images fused)
  int64_t first_pad = 0;
  int Hc = 0, Wc = 0, align_corners = 0;
  // ragged fused path (linetr_describe_ragged): the image table instead of nhwc / Hc / Wc, and the cells of all its maps
  const RaggedImage* tab = nullptr; double cells = 0;
  const BnTrain* bn = nullptr; // training-time forward (linetr_forward_train): BatchNorm on batch statistics, convolutions unfolded
  PipeStages* pipe = nullptr;  // pipelined call (linetr_describe_submit): where the launch sequence moves on to the next stream
};

bool fused_mlp_enabled(const LinetrModelConfig& c) { return c.enc_channels[1] == 64 && c.enc_channels[2] == 128; }

// rows handled by one wave of mlp123_kernel (multiples of the 32-row MFMA step).  The kernel holds 160 weights per lane,
// so one wave fits a SIMD (1024 on the chip) and workgroup dispatch is slow for such fat blocks (~10 blocks/us
// measured): give every wave one long run of rows -- a single round of <= 256 blocks -- rather than many short ones.
int mlp123_rows_per_wave(int64_t rows) {
  const int64_t waves = 256 * 4;
  return (int)std::max<int64_t>(cdiv((int)cdiv((int)rows, (int)waves), 32) * 32, 32);
}

// flops of one signature layer's attention: q k^T and p v of every (image, head)
double attn_flops(const int32_t* h_cu, int n_images) {
  double fl = 0;
  for (int i = 0; i < n_images; ++i) { const double n = h_cu[i + 1] - h_cu[i]; fl += 2.0 * 2.0 * n * n * D; }
  return fl;
}

// ---- positional encoders (up to CUT_MLP).  The word and the line encoder are the same four layers over different inputs, through
// distinct kernel instantiations; the host code below is written once and told which encoder it runs.
struct EncCall {
  int which;                   // ENC_WORD: p0 = token coordinates, p1 = scores.  ENC_LINE: p0 = sub-line end points, p1 = responses,
  const float *p0, *p1, *p2;   // p2 = (cos, sin) of the doubled angle (TokMlpArgs has the shapes)
  int64_t rows;
  float* const* act;           // FwdWs::act[which]
};
// per encoder: first-layer inputs, bytes read per row, and the profile classes of its own launches
constexpr struct { int in, in_bytes; const char *tok_mlp, *mlp123; } ENC_KIND[2] = {{3, 12, "tok_mlp_bf16x6", "mlp123"},
                                                                                   {5, 28, "line_mlp_bf16x6", "mlp123_line"}};

struct EncNorm { float cx, cy, scale; };   // normalize_keylines (line_transformer.py:30-32)
EncNorm enc_norm(const LinetrModelConfig& c) {
  return {c.norm_width / 2.f, c.norm_height / 2.f, (float)std::max(c.norm_width, c.norm_height) * 0.7f};
}

// layer 1 (no GEMM) -> out [rows, e0]; RELU = false: the pre-activations, for BatchNorm on batch statistics
template <bool RELU>
int enc_layer1(LinetrHandle* h, hipStream_t st, const EncCall& c, float* out) {
  const PosEncoder& E = h->enc[c.which];
  const EncNorm n = enc_norm(h->cfg);
  const dim3 grid((unsigned)cdiv((int)(c.rows * 8), 256));
  if (c.which == ENC_WORD)
    hipLaunchKernelGGL(word_mlp1_kernel<RELU>, grid, dim3(256), 0, st, c.p0, c.p1, c.rows, n.cx, n.cy, n.scale, E.W1, E.b1, out);
  else
    hipLaunchKernelGGL(line_mlp1_kernel<RELU>, grid, dim3(256), 0, st, c.p0, c.p1, c.p2, (int)c.rows, n.cx, n.cy, n.scale, E.W1, E.b1, out);
  LT_LAUNCH_CHECK();
  return LINETR_OK;
}

// layers 1-3 in one exact-fp32 MFMA kernel (lt_model.h) -> out [rows, e2]
int enc_mlp123(LinetrHandle* h, hipStream_t st, const EncCall& c, float* out) {
  const PosEncoder& E = h->enc[c.which];
  const EncNorm n = enc_norm(h->cfg);
  const int rpw = mlp123_rows_per_wave(c.rows);
  const dim3 grid((unsigned)cdiv((int)cdiv((int)c.rows, rpw), 4));
  if (c.which == ENC_WORD)
    hipLaunchKernelGGL(mlp123_kernel<true>, grid, dim3(256), 0, st, c.p0, c.p1, c.p2, c.rows, rpw, n.cx, n.cy, n.scale, E.W1, E.b1,
                       E.W2.W, E.W2.b, E.W3.W, E.W3.b, out);
  else
    hipLaunchKernelGGL(mlp123_kernel<false>, grid, dim3(256), 0, st, c.p0, c.p1, c.p2, c.rows, rpw, n.cx, n.cy, n.scale, E.W1, E.b1,
                       E.W2.W, E.W2.b, E.W3.W, E.W3.b, out);
  LT_LAUNCH_CHECK();
  return LINETR_OK;
}

// the operands of the one-kernel MLP (lt_tokmlp.h): layers 1-4 -> act[3]
TokMlpArgs tok_mlp_args(const LinetrHandle* h, const EncCall& c) {
  const PosEncoder& E = h->enc[c.which];
  const EncNorm n = enc_norm(h->cfg);
  TokMlpArgs a;
  a.p0 = c.p0; a.p1 = c.p1; a.p2 = c.p2; a.rows = c.rows; a.cx = n.cx; a.cy = n.cy; a.scale = n.scale;
  a.W1 = E.W1; a.b1 = E.b1; a.W2st = E.W2.st; a.b2 = E.W2.b; a.W3st = E.W3.st; a.b3 = E.W3.b; a.W4st = E.W4.st; a.b4 = E.W4.b;
  a.Y = c.act[3]; a.ldy = h->cfg.enc_channels[3];
  return a;
}

// one encoder up to its last ReLU (act[3]).  tok_mlp: layers 1-4 in one kernel; otherwise layers 1-3 in one kernel (the reference's
// channel widths) or one by one, then layer 4's GEMM
int pos_encoder(LinetrHandle* h, hipStream_t st, const EncCall& c, bool tok_mlp) {
  const int *ch = h->cfg.enc_channels, e0 = ch[0], e1 = ch[1], e2 = ch[2], e3 = ch[3];
  const PosEncoder& E = h->enc[c.which];
  const auto& kind = ENC_KIND[c.which];
  const int64_t rows = c.rows;
  int e;
  if (tok_mlp) {
    ProfScope ps(h, st, kind.tok_mlp, 2.0 * rows * (kind.in * e0 + e0 * e1 + e1 * e2 + e2 * e3), (double)rows * (kind.in_bytes + 4 * e3));
    return tok_mlp_launch(tok_mlp_args(h, c), c.which == ENC_WORD, st);
  }
  if (fused_mlp_enabled(h->cfg)) {
    ProfScope ps(h, st, kind.mlp123, 2.0 * rows * (kind.in * e0 + e0 * e1 + e1 * e2), (double)rows * (kind.in_bytes + 4 * e2));
    if ((e = enc_mlp123(h, st, c, c.act[2]))) return e;
  } else {
    {
      ProfScope ps(h, st, "mlp_first", 2.0 * rows * kind.in * e0, (double)rows * (kind.in_bytes + 4 * e0));
      if ((e = enc_layer1<true>(h, st, c, c.act[0]))) return e;
    }
    if ((e = run_gemm(h, st, E.W2, (int)rows, {c.act[0], e0}, {c.act[1], e1}, ACT_RELU))) return e;
    if ((e = run_gemm(h, st, E.W3, (int)rows, {c.act[1], e1}, {c.act[2], e2}, ACT_RELU))) return e;
  }
  return run_gemm(h, st, E.W4, (int)rows, {c.act[2], e2}, {c.act[3], e3}, ACT_RELU);
}

// one encoder in training mode (train.py:127): conv -> BatchNorm(batch statistics) -> ReLU, layer by layer, on the unfolded convolutions
// of a bn_batch_stats handle.  Statistics run over ALL rows of the batch: B*N*T token positions (padding tokens included, as the
// reference's [B*N, 3, T] input has them) for the word encoder, B*N sub-lines for the line encoder.  The encoder's four layers are
// BatchNorm layers 4 which .. 4 which + 3 of the handle; `off`: where the next layer's packed statistics go.
int pos_encoder_bn(LinetrHandle* h, hipStream_t st, const EncCall& c, const BnTrain& bt, int64_t& off) {
  const PosEncoder& E = h->enc[c.which];
  const GemmW* const W[4] = {nullptr, &E.W2, &E.W3, &E.W4};
  const int* ch = h->cfg.enc_channels;
  int e;
  for (int i = 0; i < 4; ++i) {
    e = i == 0 ? enc_layer1<false>(h, st, c, c.act[0])
               : run_gemm(h, st, *W[i], (int)c.rows, {c.act[i - 1], ch[i - 1]}, {c.act[i], ch[i]}, ACT_NONE);
    if (e) return e;
    const int layer = 4 * c.which + i;
    if ((e = bn_train_layer(st, bt, c.act[i], c.rows, ch[i], ch[i], h->bn_g[layer], h->bn_b[layer], off))) return e;
    off += 2 * ch[i];
  }
  return LINETR_OK;
}

// The token MLP's launches (the numbers are linetr_debug_tok_mlp's `variant` argument, include/linetr_hip.h)
enum { TOKV_WORD = 0, TOKV_LINE = 1, TOKV_DUAL = 2, TOKV_SEQ = 3, TOKV_CHAIN = 4 };
// What rows_word token rows and rows_line sub-lines take.  Layers 1-4 in one kernel (lt_tokmlp.h): the default precision and the
// reference's channel widths, at any size (a single pair, 4 k token rows and 400 sub-lines, gains too: 42 -> 31 us for the two
// encoders).  Each encoder takes it when its own three split-tile weight images exist (`word`, `line`); both in ONE launch only
// when both do and neither is empty (`both`: TOKV_DUAL / TOKV_SEQ, or -1: one launch sequence per encoder).
// The ONE place where the choice is made: pos_encoders and linetr_debug_tok_mlp(variant = -1) both call it.
struct TokMlpPlan { bool word, line; int both; };
bool tok_mlp_has_images(const PosEncoder& E) { return E.W2.st && E.W3.st && E.W4.st; }
TokMlpPlan tok_mlp_plan(const LinetrHandle* h, int64_t rows_word, int64_t rows_line) {
  const int* ch = h->cfg.enc_channels;
  const bool ok = fused_mlp_enabled(h->cfg) && h->precision == LINETR_PREC_BF16X6 && ch[0] == 32 && ch[1] == 64 && ch[2] == 128 && ch[3] == 256 &&
                  !LT_XENV("LINETR_NO_TOKMLP");
  TokMlpPlan p;
  p.word = ok && tok_mlp_has_images(h->enc[ENC_WORD]);
  p.line = ok && tok_mlp_has_images(h->enc[ENC_LINE]);
  p.both = !(p.word && p.line && rows_word > 0 && rows_line > 0) ? -1 : tok_mlp_dual_fits(rows_word, rows_line) ? TOKV_DUAL : TOKV_SEQ;
  return p;
}

// both encoders: the word encoder up to its last ReLU (its final linear layer is applied after pooling), the line encoder to its
// output (lpos)
int pos_encoders(LinetrHandle* h, hipStream_t& st, const TokenStage& ts, const float* sublines, const float* resp,
                 const float* angle_sub, int N, FwdWs& w) {
  const LinetrModelConfig& c = h->cfg;
  const int e0 = c.enc_channels[0], e1 = c.enc_channels[1], e2 = c.enc_channels[2], e3 = c.enc_channels[3];
  // token coordinates and scores: compact (describe) or dense (forward)
  const EncCall word{ENC_WORD, ts.cpnt ? ts.cpnt : ts.pnt, ts.cpnt ? ts.cscore : ts.score, nullptr, ts.rows, w.act[ENC_WORD]};
  const EncCall line{ENC_LINE, sublines, resp, angle_sub, N, w.act[ENC_LINE]};
  const int64_t rows = ts.rows;
  int e;
  const TokMlpPlan plan = tok_mlp_plan(h, rows, N);
  if (ts.bn) {
    int64_t off = 0;
    if ((e = pos_encoder_bn(h, st, word, *ts.bn, off))) return e;
    if ((e = pos_encoder_bn(h, st, line, *ts.bn, off))) return e;
  } else if (plan.both >= 0) {
    // side by side for a small batch, one after the other inside every persistent block for a large one
    ProfScope ps(h, st, "pos_mlp_dual_bf16x6", 2.0 * rows * (3 * e0 + e0 * e1 + e1 * e2 + e2 * e3) + 2.0 * N * (5 * e0 + e0 * e1 + e1 * e2 + e2 * e3),
                 (double)rows * (12 + 4 * e3) + (double)N * (28 + 4 * e3));
    if ((e = tok_mlp_launch_dual(tok_mlp_args(h, word), tok_mlp_args(h, line), st))) return e;
  } else {
    if ((e = pos_encoder(h, st, word, plan.word))) return e;
    if ((e = pos_encoder(h, st, line, plan.line))) return e;
  }
  return run_gemm(h, st, h->lW5, N, {w.act[ENC_LINE][3], e3}, {w.lpos, D}, ACT_NONE);
}

// ---- CLS-row attention pooling + value / last-MLP projection (up to CUT_POOL)
// The pooling kernels (the numbers are linetr_debug_cls_pool's `kernel` argument, include/linetr_hip.h)
enum { POOLK_DENSE = 0, POOLK_ONLINE = 1, POOLK_ONLINE_REV = 2, POOLK_SPLIT4 = 3 };
// The ONE place where the choice is made (cls_pooling and linetr_debug_cls_pool(kernel = -1) both call it): the dense token stage
// has one kernel; of the online kernels, few sub-lines (a single pair) take four waves per sub-line, so that the chip is covered
// and the token chain is a quarter as long, many take one wave per sub-line, the last sub-lines first (see the kernel)
int cls_pool_plan(bool online, int N) { return !online ? POOLK_DENSE : N <= 2048 ? POOLK_SPLIT4 : POOLK_ONLINE_REV; }

// kernel `kernel` over the token stage ts and the word encoder's activations a4 -> pooled [N][4][544]
int cls_pool_launch(LinetrHandle* h, hipStream_t st, int kernel, const TokenStage& ts, int n_images, int N, int T, const float* a4,
                    float* pooled) {
  const int64_t rows = ts.rows;
  if (kernel != POOLK_DENSE) {
    // algorithmic bytes: the dense map once (or the four taps of every token, whichever is less), one a4 row per token, the pooled rows out
    const double map_cells = ts.tab ? ts.cells : (double)n_images * ts.Hc * ts.Wc;   // ragged: summed over the table
    const double esize = ts.map_type == MT_F32 ? 4 : 2;
    const double tap_bytes = std::min(map_cells * D * esize, (double)rows * D * esize * 4);
    ProfScope ps(h, st, "cls_pool_online", 2.0 * rows * (2.0 * HEADS * D * 2), tap_bytes + (double)rows * D * 4 + (double)N * HEADS * POOLW * 4);
    if (ts.tab && kernel == POOLK_SPLIT4)
      LT_LAUNCH_BY_ELEM(ts.map_type, cls_pool_online_ragged_kernel<4>, (cls_pool_online_ragged_typed_kernel<4, E>), dim3(N), dim3(256), 0, st,
                        ts.recs, ts.sub2line_g, ts.cpnt, a4, ts.first_pad, N, T, ts.tab, ts.align_corners, h->pool, pooled, 0);
    else if (ts.tab)
      LT_LAUNCH_BY_ELEM(ts.map_type, cls_pool_online_ragged_kernel<1>, (cls_pool_online_ragged_typed_kernel<1, E>), dim3(cdiv(N, 4)), dim3(256),
                        0, st, ts.recs, ts.sub2line_g, ts.cpnt, a4, ts.first_pad, N, T, ts.tab, ts.align_corners, h->pool, pooled,
                        kernel == POOLK_ONLINE_REV ? 1 : 0);
    else if (kernel == POOLK_SPLIT4)
      LT_LAUNCH_BY_ELEM(ts.map_type, cls_pool_online_kernel<4>, (cls_pool_online_typed_kernel<4, E>), dim3(N), dim3(256), 0, st, ts.recs,
                        ts.sub2line_g, ts.cpnt, a4, ts.first_pad, N, T, (const E*)ts.nhwc, ts.Hc, ts.Wc, ts.align_corners, h->pool, pooled, 0);
    else
      LT_LAUNCH_BY_ELEM(ts.map_type, cls_pool_online_kernel<1>, (cls_pool_online_typed_kernel<1, E>), dim3(cdiv(N, 4)), dim3(256), 0, st,
                        ts.recs, ts.sub2line_g, ts.cpnt, a4, ts.first_pad, N, T, (const E*)ts.nhwc, ts.Hc, ts.Wc, ts.align_corners, h->pool,
                        pooled, kernel == POOLK_ONLINE_REV ? 1 : 0);
    LT_LAUNCH_CHECK();
  } else {
    ProfScope ps(h, st, "cls_pool", 2.0 * rows * (2.0 * HEADS * D * 2), (double)rows * D * 8);
    hipLaunchKernelGGL(cls_pool_kernel, dim3(N), dim3(256), HEADS * (T + 1) * sizeof(float), st, ts.desc, a4, T, h->pool, pooled);
    LT_LAUNCH_CHECK();
  }
  return LINETR_OK;
}

// value / last-MLP projection of the pooled rows [N][4][544] -> att [N][256] (cls_pooling and linetr_debug_stage both call it):
// one product per head, the head's DH rows of Watt over its pooled row
int value_projection(LinetrHandle* h, hipStream_t st, int N, const float* pooled, float* att) {
  const GemmGroups heads{HEADS, DH, POOLW, DH};
  return run_gemm(h, st, h->Watt, N, {pooled, HEADS * POOLW}, {att, D}, ACT_NONE, nullptr, &heads);
}

int cls_pooling(LinetrHandle* h, hipStream_t& st, const TokenStage& ts, int n_images, int N, int T, FwdWs& w) {
  if (int e = cls_pool_launch(h, st, cls_pool_plan(ts.cpnt != nullptr, N), ts, n_images, N, T, w.act[ENC_WORD][3], w.pooled)) return e;
  return value_projection(h, st, N, w.pooled, w.att);
}

// ---- the descriptive layer's tail (up to CUT_SENTENCE): the sentence rows zA, input of the line-signature network
int sentence(LinetrHandle* h, hipStream_t& st, int N, FwdWs& w) {
  const LinetrModelConfig& c = h->cfg;
  int e;
  {  // o = LN(fc(att) + cls)  (line_attention.py:36-40; the CLS residual sits in the bias)
    NormSpec ns; ns.mode = 1; ns.gamma = h->ln1g; ns.beta = h->ln1b; ns.eps = 1e-6f;
    if ((e = run_gemm_norm(h, st, h->Wfc, N, {w.att, D}, nullptr, w.fc, w.o, ns))) return e;
  }
  if ((e = run_gemm(h, st, h->Wf1, N, {w.o, D}, {w.f1, c.d_inner}, ACT_GELU))) return e;
  // sentence = line_pos + LN(w_2(gelu(w_1 o)) + o)  (line_attention.py:79-83, line_transformer.py:128)
  NormSpec ns; ns.mode = 1; ns.gamma = h->ln2g; ns.beta = h->ln2b; ns.add2 = w.lpos; ns.eps = 1e-6f;
  return run_gemm_norm(h, st, h->Wf2, N, {w.f1, c.d_inner}, w.o, w.f2, w.zA, ns);
}

// The signature attention's kernels (the numbers are linetr_debug_sig_attention's `kernel` argument, include/linetr_hip.h)
enum { SIGK_F32 = 0, SIGK_SMALL = 1, SIGK_SPLIT4 = 2, SIGK_SPLIT8 = 3, SIGK_FUSED = 4 };
// What a batch of n_images images, N sub-lines in all and max_n in the largest takes: `attn` is the kernel that reads q/k/v rows,
// `fused` replaces it and the projection GEMM by sig_qkv_attn_kernel, `fold_next` makes the next layer's q/k/v with x_out.
struct SigAttnPlan {
  int attn;
  bool fold_next, fused;
  bool eight_waves = false;   // forced plans only (LINETR_SIG_EIGHT_WAVES): the fused kernel's eight-compute-wave form at any size
  int kernel() const { return fused ? SIGK_FUSED : attn; }
};
// The ONE place where the choice is made: sig_network and linetr_debug_sig_attention(kernel = -1) both call it.
SigAttnPlan sig_attn_plan(const LinetrHandle* h, int n_images, int N, int max_n) {
  SigAttnPlan p;
  // small: few (image, head) pairs, 32-query blocks whose 4 waves also split the KV range (a single pair spreads over 56 CUs and
  // the critical path is 2 KV chunks instead of 7)
  const bool small_attn = h->precision != LINETR_PREC_F32 && (int64_t)n_images * HEADS * cdiv(max_n, 256) < 64;
  p.attn = h->precision == LINETR_PREC_F32 ? SIGK_F32 : small_attn ? SIGK_SMALL : max_n <= 128 ? SIGK_SPLIT4 : SIGK_SPLIT8;
  // single-pair sizes (the 32-query attention is taken): x_out and the NEXT layer's q/k/v come out of ONE contraction over
  // [z ; hid] (SigLayer::Wnext) -- one dependent launch less per layer where a launch costs more than its flops
  p.fold_next = small_attn && N <= SIG_FOLD_MAX_ROWS && !LT_XENV("LINETR_NO_SIG_FOLD");
  // fused q/k/v projection + attention: images of up to 256 sub-lines, and enough (image, head) blocks to fill the chip
  p.fused = !p.fold_next && !LT_XENV("LINETR_NO_FUSED_QKV_ATTN") && h->precision == LINETR_PREC_BF16X6 && max_n <= 256 &&
            (int64_t)n_images * HEADS >= 128;
  return p;
}

// Can sig_network run plan `p`, chosen by hand (linetr_debug_stage), on this batch?  What its buffers and kernels cannot serve is
// refused here, before anything is launched; every plan sig_attn_plan makes passes.
int sig_plan_servable(const LinetrHandle* h, const SigAttnPlan& p, int N, int max_n) {
  if (p.attn < SIGK_F32 || p.attn > SIGK_SPLIT8) return fail(LINETR_E_ARG, "sig plan: attention kernel %d outside 0 .. 3", p.attn);
  if (h->precision == LINETR_PREC_F32 && (p.attn != SIGK_F32 || p.fused))
    return fail(LINETR_E_ARG, "sig plan: the f32 mode runs sig_attn_kernel (0) only");
  if (p.fold_next) {
    if (p.fused) return fail(LINETR_E_ARG, "sig plan: fold_next and the fused projection + attention exclude each other");
    if (p.attn != SIGK_SMALL) return fail(LINETR_E_ARG, "sig plan: fold_next leaves q/k/v at row stride 1024, which sig_attn_small (1) alone reads");
    if (N > SIG_FOLD_MAX_ROWS) return fail(LINETR_E_ARG, "sig plan: fold_next has buffers for up to %d sub-lines (got %d)", SIG_FOLD_MAX_ROWS, N);
  }
  if (p.fused) {
    if (h->precision != LINETR_PREC_BF16X6) return fail(LINETR_E_ARG, "sig plan: the fused projection + attention runs in bf16x6 mode only");
    if (max_n > 256) return fail(LINETR_E_ARG, "sig plan: the fused projection + attention takes images of up to 256 sub-lines (got %d)", max_n);
    for (const SigLayer& S : h->sig)
      if (!S.Wqkv.st) return fail(LINETR_E_ARG, "sig plan: a layer has no split-tile weight image for the fused projection + attention");
  }
  return LINETR_OK;
}

// one signature layer's attention by kernel `kernel` (SIGK_F32 .. SIGK_SPLIT8), q/k/v rows at qkv (row stride ldq) -> msg: exact-fp32
// MFMA attention (f32 mode), fp32-faithful split-bf16 (6 products) otherwise.  SIGK_SMALL is the only kernel that takes ldq != 3 D.
int sig_attention(LinetrHandle* h, hipStream_t st, int kernel, const float* qkv, int ldq, const int* cu_dev, int n_images, int N,
                  int max_n, double fl, float* msg) {
  if (kernel == SIGK_F32) {
    ProfScope ps(h, st, "sig_attn", fl, (double)N * D * 16);
    hipLaunchKernelGGL(sig_attn_kernel, dim3(n_images, HEADS, cdiv(max_n, ATT_QT)), dim3(256), 0, st, qkv, cu_dev, msg);
  } else {
    ProfScope ps(h, st, "sig_attn_bf16x6", fl, (double)N * D * 16);
    if (kernel == SIGK_SMALL)
      // (r04: an eight-wave form -- one key chunk per wave, K fragments straight from global memory -- measured level with this
      // one, 12.6 us per launch for a cfg2 pair either way, and was not kept)
      hipLaunchKernelGGL(sig_attn_small_kernel, dim3(n_images, HEADS, cdiv(max_n, 32)), dim3(256), 0, st, qkv, cu_dev, msg, ldq);
    else if (kernel == SIGK_SPLIT4)
      hipLaunchKernelGGL(sig_attn_split_kernel<4>, dim3(n_images, HEADS, cdiv(max_n, ATT_QT)), dim3(256), 0, st, qkv, cu_dev, msg);
    else
      hipLaunchKernelGGL(sig_attn_split_kernel<8>, dim3(n_images, HEADS, cdiv(max_n, 256)), dim3(512), 0, st, qkv, cu_dev, msg);
  }
  LT_LAUNCH_CHECK();
  return LINETR_OK;
}

// q/k/v projection + attention of an (image, head) in one launch (lt_attn_fused.h), z -> msg: q, k, v never reach HBM
// Images of up to 224 sub-lines leave the eighth wave without rows: it becomes the ring's only DMA issuer (the producer form) and
// the seven others keep MFMAs, LDS reads and the split in their loop.  Larger images, or `eight_waves` (a forced plan of the debug
// entry points), take the form in which all eight waves compute and each issues its share.  Same bits either way.
int sig_qkv_attention(LinetrHandle* h, hipStream_t st, const SigLayer& S, const float* z, const int* cu_dev, int n_images, int N,
                      int max_n, bool eight_waves, double attn_fl, float* msg) {
  const bool producer = !eight_waves && max_n <= FQA_PRODUCER_ROWS;
  LT_HIP(producer ? allow_dynamic_lds<sig_qkv_attn_kernel<true>>(FQA_LDS) : allow_dynamic_lds<sig_qkv_attn_kernel<false>>(FQA_LDS));
  ProfScope ps(h, st, "sig_qkv_attn_bf16x6", 2.0 * N * 3.0 * D * D + attn_fl, (double)N * D * 8);
  hipLaunchKernelGGL(producer ? sig_qkv_attn_kernel<true> : sig_qkv_attn_kernel<false>, dim3(n_images, HEADS), dim3(512), FQA_LDS,
                     st, z, S.Wqkv.st, S.Wqkv.b, cu_dev, msg);
  LT_LAUNCH_CHECK();
  return LINETR_OK;
}

// ---- line-signature network + final projection and L2 normalisation (CUT_SIG0 + l behind layer l).
// models/line_transformer.py:132-183, 245-246
// `forced` (linetr_debug_stage only, checked by sig_plan_servable): the plan to run instead of sig_attn_plan's; w.tap (the same
// caller only): where x_out behind every layer but the last is copied.  Every product call leaves both null.
int sig_network(LinetrHandle* h, hipStream_t& st, const TokenStage& ts, const int32_t* h_cu, const int* cu_dev, int n_images, int N,
                float* d_line_desc, FwdWs& w, const SigAttnPlan* forced = nullptr) {
  const LinetrModelConfig& c = h->cfg;
  int max_n = 0;
  for (int i = 0; i < n_images; ++i) max_n = std::max(max_n, h_cu[i + 1] - h_cu[i]);
  int e;
  const double attn_fl = attn_flops(h_cu, n_images);
  // the signature layers' slots behind the two encoders' in the packed BatchNorm statistics
  const int64_t sig_bn_off = 4 * (int64_t)(c.enc_channels[0] + c.enc_channels[1] + c.enc_channels[2] + c.enc_channels[3]);
  const SigAttnPlan plan = forced ? *forced : sig_attn_plan(h, n_images, N, max_n);
  const bool fold_next = plan.fold_next, fused_qkv_attn = plan.fused;
  float *z = w.zA, *zn = w.zB;     // the layer's input rows (row stride ldz) and the next layer's
  int ldz = D;
  float *zq = w.zqA, *zq_next = w.zqB;   // fold_next: [x_out | q/k/v of the next layer] rows; z is the head of one (ldz = 4 D)
  const float* qkv = w.qkv;        // where the layer's q/k/v sit, and their row stride
  int ldq = 3 * D;
  for (size_t l = 0; l < h->sig.size(); ++l) {
    const SigLayer& S = h->sig[l];
    if (fused_qkv_attn && S.Wqkv.st) {
      if ((e = sig_qkv_attention(h, st, S, z, cu_dev, n_images, N, max_n, plan.eight_waves, attn_fl, w.msgp))) return e;
    } else {
      // (with fold_next the previous layer has made them already)
      if (!fold_next || l == 0)
        if ((e = run_gemm(h, st, S.Wqkv, N, {z, ldz}, {w.qkv, 3 * D}, ACT_NONE))) return e;
      if ((e = sig_attention(h, st, plan.attn, qkv, ldq, cu_dev, n_images, N, max_n, attn_fl, w.msgp))) return e;
    }
    if ((e = run_gemm(h, st, S.W1, N, {z, ldz, w.msgp, D, D}, {w.hid, 2 * D}, ts.bn ? ACT_NONE : ACT_RELU))) return e;
    if (ts.bn && (e = bn_train_layer(st, *ts.bn, w.hid, N, 2 * D, 2 * D, h->bn_g[8 + l], h->bn_b[8 + l], sig_bn_off + (int64_t)l * 4 * D))) return e;
    if (l + 1 == h->sig.size()) break;   // the last layer's second MLP GEMM is folded into the final projection below
    if (fold_next) {
      if ((e = run_gemm(h, st, S.Wnext, N, {z, ldz, w.hid, 2 * D, D}, {zq, 4 * D}, ACT_NONE))) return e;
      z = zq; ldz = 4 * D; qkv = zq + D; ldq = 4 * D;
      std::swap(zq, zq_next);
    } else {
      if ((e = run_gemm(h, st, S.W2, N, {w.hid, 2 * D}, {zn, D}, ACT_NONE, z))) return e;
      std::swap(z, zn);
    }
    if (w.tap)
      LT_HIP(hipMemcpy2DAsync(w.tap + (int64_t)l * N * D, D * sizeof(float), z, ldz * sizeof(float), D * sizeof(float), N,
                              hipMemcpyDeviceToDevice, st));
    if ((e = pipe_boundary(ts.pipe, CUT_SIG0 + (int)l, st))) return e;
  }
  NormSpec l2; l2.mode = 2;      // F.normalize(final_proj(.), dim=1)  (line_transformer.py:245-246)
  if (h->sig.empty()) return run_gemm_norm(h, st, h->Wfin, N, {z, D}, nullptr, zn, d_line_desc, l2);
  // final_proj(z + W2 hid + b2) = [Wfin | Wfin W2] [z ; hid] + (Wfin b2 + bfin): one K = 768 GEMM instead of two launches
  return run_gemm_norm(h, st, h->Wfin2, N, {z, ldz, w.hid, 2 * D, D}, nullptr, zn, d_line_desc, l2);
}
}  // namespace

#ifdef LINETR_EXPERIMENTS
#include "lt_x_net.h"
#endif

namespace {
int forward_core(LinetrHandle* h, hipStream_t st, const TokenStage& ts, const float* sublines, const float* resp,
                 const float* angle_sub, const int32_t* h_cu, const int* cu_dev, int n_images, int N, int T,
                 float* d_line_desc, FwdWs& w) {
  int e;
#ifdef LINETR_EXPERIMENTS
  XPath xp;   // which path takes the signature network (lt_x_net.h)
  if ((e = x_begin(h, st, n_images, N, h_cu, w, xp))) return e;
#endif
  if ((e = pos_encoders(h, st, ts, sublines, resp, angle_sub, N, w))) return e;
  if ((e = pipe_boundary(ts.pipe, CUT_MLP, st))) return e;
  if ((e = cls_pooling(h, st, ts, n_images, N, T, w))) return e;
  if ((e = pipe_boundary(ts.pipe, CUT_POOL, st))) return e;
#ifdef LINETR_EXPERIMENTS
  if (xp != X_NONE) return x_rest(h, st, ts, h_cu, cu_dev, n_images, N, d_line_desc, w, xp);
#endif
  if ((e = sentence(h, st, N, w))) return e;
  if ((e = pipe_boundary(ts.pipe, CUT_SENTENCE, st))) return e;
  return sig_network(h, st, ts, h_cu, cu_dev, n_images, N, d_line_desc, w);
}

int check_cu(const int32_t* h_cu, int n_images) {
  if (!h_cu || n_images < 1) return fail(LINETR_E_ARG, "null / empty cu_sub");
  if (h_cu[0] != 0) return fail(LINETR_E_ARG, "cu_sub[0] != 0");
  for (int i = 0; i < n_images; ++i)
    if (h_cu[i + 1] < h_cu[i]) return fail(LINETR_E_ARG, "cu_sub not monotone");
  return 0;
}

// the sub-line prefix sums on the device: the caller's copy, or h_cu uploaded into the workspace
int cu_on_device(const int32_t* h_cu, const int32_t* d_cu, int n_images, const FwdWs& w, hipStream_t st, const int*& cu_dev) {
  cu_dev = d_cu;
  if (cu_dev) return LINETR_OK;
  LT_HIP(hipMemcpyAsync(w.cu, h_cu, (n_images + 1) * sizeof(int), hipMemcpyHostToDevice, st));
  cu_dev = w.cu;
  return LINETR_OK;
}

// linetr_forward (bt = nullptr) and linetr_forward_train (bt: running / batch statistics and momentum set by the caller; its scratch
// sits behind linetr_forward's workspace) behind their own argument checks: the network over the reference's dense [N, T] token tensors
int forward_dense(LinetrHandle* h, const char* who, const LinetrTokens& tok, const int32_t* h_cu, const int32_t* d_cu, int n_images,
                  int T, float* d_line_desc, void* d_ws, int64_t ws_bytes, hipStream_t st, BnTrain* bt) {
  if (int e = check_cu(h_cu, n_images)) return e;
  const int N = h_cu[n_images];
  if (N <= 0) return LINETR_OK;
  if (!tok.sublines || !tok.pnt || !tok.resp || !tok.angle_sub || !tok.desc || !tok.score || !d_line_desc)
    return fail(LINETR_E_ARG, "%s: null tensor", who);
  if (ws_bytes < (bt ? linetr_forward_train_workspace_bytes(h, N, T) : linetr_forward_workspace_bytes(h, N, T)))
    return fail(LINETR_E_WORKSPACE, "%s: workspace too small", who);
  if ((int64_t)N * T > INT32_MAX / 8) return fail(LINETR_E_ARG, "%s: batch too large", who);
  LT_HIP(hipSetDevice(h->device));
  FwdWs w = fwd_layout(h, N, (int64_t)N * T, std::max(N, 1), (char*)d_ws);
  if (bt) {
    bt->partial = (double*)((char*)d_ws + align_up(w.total, 256));
    bt->affine = (float*)((char*)bt->partial + (int64_t)BN_MAX_BLOCKS * 2 * BN_MAX_CHANNELS * 8);
  }
  const int* cu_dev;
  if (int e = cu_on_device(h_cu, d_cu, n_images, w, st, cu_dev)) return e;
  TokenStage ts;
  ts.pnt = tok.pnt; ts.score = tok.score; ts.desc = tok.desc; ts.rows = (int64_t)N * T;
  ts.bn = bt;
  return forward_core(h, st, ts, tok.sublines, tok.resp, tok.angle_sub, h_cu, cu_dev, n_images, N, T, d_line_desc, w);
}
}  // namespace

extern "C" int linetr_forward(LinetrHandle* h, const LinetrTokens* tok, const int32_t* h_cu, const int32_t* d_cu,
                              int32_t n_images, int32_t T, float* d_line_desc, void* d_ws, int64_t ws_bytes,
                              void* stream) {
  if (!h || !tok) return fail(LINETR_E_ARG, "forward: null argument");
  if (h->cfg.bn_batch_stats) return fail(LINETR_E_ARG, "forward: a training-mode handle (bn_batch_stats = 1) runs linetr_forward_train only");
  return forward_dense(h, "forward", *tok, h_cu, d_cu, n_images, T, d_line_desc, d_ws, ws_bytes, (hipStream_t)stream, nullptr);
}

// Training-time forward (train.py:127,163-164): linetr_forward's dense token path with BatchNorm on batch
// statistics (lt_bntrain.h).  The workspace is linetr_forward's plus the statistics scratch.
extern "C" int64_t linetr_bn_stats_floats(const LinetrHandle* h) {
  if (!h) return -1;
  const LinetrModelConfig& c = h->cfg;
  return 4 * (int64_t)(c.enc_channels[0] + c.enc_channels[1] + c.enc_channels[2] + c.enc_channels[3]) + (int64_t)c.n_sig_layers * 4 * D;
}

extern "C" int64_t linetr_forward_train_workspace_bytes(const LinetrHandle* h, int32_t N, int32_t T) {
  if (!h) return -1;
  return linetr_forward_workspace_bytes(h, N, T) + (int64_t)BN_MAX_BLOCKS * 2 * BN_MAX_CHANNELS * 8 + 2 * BN_MAX_CHANNELS * 4 + 512;
}

extern "C" int linetr_forward_train(LinetrHandle* h, const LinetrTokens* tok, const int32_t* h_cu, const int32_t* d_cu, int32_t n_images,
                                    int32_t T, float momentum, float* d_bn_running, float* d_bn_batch, float* d_line_desc, void* d_ws,
                                    int64_t ws_bytes, void* stream) {
  if (!h || !tok) return fail(LINETR_E_ARG, "forward_train: null argument");
  if (!h->cfg.bn_batch_stats) return fail(LINETR_E_ARG, "forward_train: the handle was created for inference (bn_batch_stats = 0)");
  if (!d_bn_running) return fail(LINETR_E_ARG, "forward_train: null running statistics");
  if (!(momentum >= 0.f && momentum <= 1.f)) return fail(LINETR_E_ARG, "forward_train: momentum out of [0, 1]");
  BnTrain bt;
  bt.running = d_bn_running; bt.batch = d_bn_batch; bt.momentum = momentum;
  return forward_dense(h, "forward_train", *tok, h_cu, d_cu, n_images, T, d_line_desc, d_ws, ws_bytes, (hipStream_t)stream, &bt);
}

// =============================================================================================
// fused tokenise + describe
// =============================================================================================

namespace {
struct DescWs { void* nhwc; float *cpnt, *cscore, *sublines, *resp, *angle_sub; int* s2l_g; int64_t fwd_off, total; };
DescWs desc_layout(int n_images, int height, int width, int N, int64_t rows, char* base) {
  DescWs d;
  int64_t off = 0;
  auto take = [&](int64_t bytes) { char* p = base + off; off += align_up(bytes, 256); return p; };
  const int64_t P = (int64_t)(height / 8) * (width / 8);
  d.nhwc = take(n_images * P * D * 4);   // (sized for float32: a half copy fills half of it)
  d.cpnt = (float*)take(rows * 8);
  d.cscore = (float*)take(rows * 4);
  d.sublines = (float*)take((int64_t)N * 16);
  d.resp = (float*)take((int64_t)N * 4);
  d.angle_sub = (float*)take((int64_t)N * 8);
  d.s2l_g = (int*)take((int64_t)N * 4);
  d.fwd_off = off;
  d.total = off;
  return d;
}
}  // namespace

extern "C" int64_t linetr_describe_workspace_bytes(const LinetrHandle* h, int32_t n_images, int32_t height, int32_t width,
                                                   int32_t N, int64_t n_real) {
  if (!h) return -1;
  const int64_t rows = n_real + n_images;
  return desc_layout(n_images, height, width, std::max(N, 1), rows, nullptr).total +
         fwd_layout(h, std::max(N, 1), rows, n_images, nullptr).total;
}

namespace {
// The launches of a describe call behind its argument checks: the token front `f` (its geometry set by the caller: one size for the
// batch, or the image table), then the network.  `dw` / `fwd_base`: the workspace behind whatever the caller put in front of it.
int describe_launch(LinetrHandle* h, hipStream_t st, TokenFront f, const DescWs& dw, char* fwd_base, const LinetrTokens& out,
                    const K2sTable& k2s, int32_t* d_sub2line, float* d_line_desc, const int32_t* h_cu, const int32_t* d_cu, int64_t n_real,
                    PipeStages* pipe) {
  const int n_images = f.n_images, N = f.N;
  const int64_t rows = n_real + n_images;
  FwdWs w = fwd_layout(h, N, rows, n_images, fwd_base);
  const int* cu_dev;
  if (int e = cu_on_device(h_cu, d_cu, n_images, w, st, cu_dev)) return e;
  f.sublines = out.sublines ? out.sublines : dw.sublines;
  f.resp = out.resp ? out.resp : dw.resp;
  f.angle_sub = out.angle_sub ? out.angle_sub : dw.angle_sub;
  f.s2l_g = dw.s2l_g; f.nhwc_buf = dw.nhwc;
  f.map_always = true;
  f.tokenize_bytes = (double)n_real * 16;
  f.cpnt = dw.cpnt; f.cscore = dw.cscore; f.n_pad_images = n_images; f.first_pad = n_real;
  const void* nhwc_map;
  if (int e = token_front(h, st, f, out, k2s, d_sub2line, nhwc_map)) return e;
  TokenStage ts;
  ts.cpnt = dw.cpnt; ts.cscore = dw.cscore; ts.nhwc = nhwc_map; ts.map_type = f.mf.type; ts.recs = f.recs; ts.sub2line_g = dw.s2l_g;
  ts.rows = rows; ts.first_pad = n_real; ts.Hc = f.height / 8; ts.Wc = f.width / 8; ts.align_corners = f.align_corners;
  ts.tab = f.tab; ts.cells = f.cells;
  ts.pipe = pipe;
  if (int e = pipe_boundary(pipe, CUT_TOKENS, st)) return e;
  return forward_core(h, st, ts, f.sublines, f.resp, f.angle_sub, h_cu, cu_dev, n_images, N, f.T, d_line_desc, w);
}

// linetr_describe proper.  pipe != nullptr (linetr_describe_submit): the launch sequence moves from stream to stream at the plan's
// cut points; `st` is the first stage's stream.
int describe_impl(LinetrHandle* h, const LinetrLineRec* d_recs, int32_t K, int32_t N, int64_t n_real,
                  const int32_t* h_cu, const int32_t* d_cu, int32_t n_images, double td, int32_t T,
                  const void* d_dense_desc, const float* d_dense_score, int32_t height, int32_t width,
                  int32_t align_corners, int32_t dense_is_nhwc, const LinetrTokens& out, int32_t* d_sub2line,
                  float* d_line_desc, void* d_ws, int64_t ws_bytes, hipStream_t st, PipeStages* pipe) {
  if (!h) return fail(LINETR_E_ARG, "describe: null handle");
  if (h->cfg.bn_batch_stats) return fail(LINETR_E_ARG, "describe: a training-mode handle (bn_batch_stats = 1) runs linetr_forward_train only");
  if (int e = check_cu(h_cu, n_images)) return e;
  if (h_cu[n_images] != N) return fail(LINETR_E_ARG, "describe: cu_sub does not end at N");
  if (K <= 0 || N <= 0) return LINETR_OK;
  if (!d_recs || !d_dense_desc || !d_dense_score || !d_line_desc || !d_ws) return fail(LINETR_E_ARG, "describe: null pointer");
  if (T < 1 || T > 4096 || height % 8 || width % 8) return fail(LINETR_E_ARG, "describe: bad max_tokens / image size");
  if (n_real < N || n_real > (int64_t)N * T) return fail(LINETR_E_ARG, "describe: implausible real-token count");
  if (out.desc && !out.pnt) return fail(LINETR_E_ARG, "describe: out.desc requires out.pnt");
  MapFormat mf;
  if (int e = map_format(dense_is_nhwc, "describe", mf)) return e;
  if (!mf.aligned(d_dense_desc) || !aligned16(out.desc) || !aligned16(d_ws))
    return fail(LINETR_E_ARG, "describe: a channel-last descriptor map, out.desc and the workspace must be 16-byte aligned (a half channel-last map: 8-byte)");
  K2sTable k2s;
  if (int e = k2s_table(out, n_images, K, N, h_cu, k2s, "describe")) return e;
  if (ws_bytes < linetr_describe_workspace_bytes(h, n_images, height, width, N, n_real))
    return fail(LINETR_E_WORKSPACE, "describe: workspace too small");
  const int64_t rows = n_real + n_images;
  if (rows > INT32_MAX / 8) return fail(LINETR_E_ARG, "describe: batch too large");
  LT_HIP(hipSetDevice(h->device));
  DescWs dw = desc_layout(n_images, height, width, N, rows, (char*)d_ws);
  TokenFront f{d_recs, K, N, td, T, d_dense_desc, d_dense_score, n_images, height, width, align_corners, mf,
               (double)width - 0.6, (double)height - 0.6};
  return describe_launch(h, st, f, dw, (char*)d_ws + dw.fwd_off, out, k2s, d_sub2line, d_line_desc, h_cu, d_cu, n_real, pipe);
}

// Workspace of linetr_describe_ragged in front of linetr_describe's own segments: image table | channel-last copy of every NCHW-fed
// map.  The ONE function that lays it out and the one that makes the table: the size query passes no table, the entry point the
// host copy it uploads (`base`: where the workspace is on the device).
struct RaggedFront { int64_t o_tab, total; int max_cells; double cells; };
RaggedFront ragged_front(const LinetrImage* imgs, int n_images, const MapFormat& mf, char* base, RaggedImage* tab) {
  RaggedFront L{};
  Carve c;
  L.o_tab = c.take(sz_mul(n_images, sizeof(RaggedImage)));
  for (int i = 0; i < n_images; ++i) {
    const LinetrImage& im = imgs[i];
    const int Hc = im.height / 8, Wc = im.width / 8;
    const int64_t o_copy = mf.nhwc ? 0 : c.take(sz_mul(Hc, Wc, D * mf.esize));
    L.max_cells = std::max(L.max_cells, Hc * Wc);
    L.cells += (double)Hc * Wc;
    if (tab)
      tab[i] = RaggedImage{mf.nhwc ? im.d_dense_desc : (const void*)(base + o_copy), im.d_dense_score,
                           mf.nhwc ? nullptr : im.d_dense_desc, im.height, im.width, Hc, Wc, im.token_distance,
                           (double)im.width - 0.6, (double)im.height - 0.6};
  }
  L.total = c.o;
  return L;
}
// what the table must be like for ragged_front's arithmetic to mean anything (the query answers 0 otherwise, the entry point refuses)
int check_images(const LinetrImage* imgs, int n_images, int dense_is_nhwc, MapFormat& mf) {
  if (int e = map_format(dense_is_nhwc, "describe_ragged", mf)) return e;
  if (!imgs || n_images < 1) return fail(LINETR_E_ARG, "describe_ragged: a NULL or empty image table");
  for (int i = 0; i < n_images; ++i) {
    const LinetrImage& im = imgs[i];
    if (im.height <= 0 || im.width <= 0 || im.height % 8 || im.width % 8)
      return fail(LINETR_E_ARG, "describe_ragged: image %d is %d x %d, not a positive multiple of 8 each way", i, im.height, im.width);
    if ((int64_t)(im.height / 8) * (im.width / 8) > INT32_MAX / D) return fail(LINETR_E_ARG, "describe_ragged: image %d is too large", i);
    if (!im.d_dense_desc || !im.d_dense_score) return fail(LINETR_E_ARG, "describe_ragged: image %d has a NULL map", i);
    if (!mf.aligned(im.d_dense_desc))
      return fail(LINETR_E_ARG, "describe_ragged: the channel-last descriptor map of image %d is not 16-byte aligned (a half channel-last map: 8-byte; an NCHW map: its element)", i);
    if (!(im.token_distance > 0)) return fail(LINETR_E_ARG, "describe_ragged: image %d: token_distance must be > 0", i);
  }
  return 0;
}
}  // namespace

// the whole workspace of a checked table, saturating (SZ_LIMIT: a shape no call serves): what the query answers and the call compares
static int64_t describe_ragged_total(const LinetrHandle* h, const LinetrImage* h_images, int n_images, const MapFormat& mf, int N, int64_t n_real) {
  const int64_t rows = n_real + n_images;
  return sz_add(ragged_front(h_images, n_images, mf, nullptr, nullptr).total,
                desc_layout(0, 0, 0, std::max(N, 1), rows, nullptr).total, fwd_layout(h, std::max(N, 1), rows, n_images, nullptr).total);
}

extern "C" int64_t linetr_describe_ragged_workspace_bytes(const LinetrHandle* h, const LinetrImage* h_images, int32_t n_images,
                                                          int32_t dense_is_nhwc, int32_t N, int64_t n_real) {
  MapFormat mf;
  if (!h || check_images(h_images, n_images, dense_is_nhwc, mf)) return -1;
  return sz_answer(describe_ragged_total(h, h_images, n_images, mf, N, n_real));
}

extern "C" int linetr_describe_ragged(LinetrHandle* h, const LinetrLineRec* d_recs, const LinetrLineRec* h_recs, int32_t K, int32_t N,
                                      int64_t n_real, const int32_t* h_cu, const int32_t* d_cu, const LinetrImage* h_images,
                                      int32_t n_images, int32_t T, int32_t align_corners, int32_t dense_is_nhwc, LinetrTokens out,
                                      int32_t* d_sub2line, float* d_line_desc, void* d_ws, int64_t ws_bytes, void* stream) {
  if (!h) return fail(LINETR_E_ARG, "describe_ragged: null handle");
  if (h->cfg.bn_batch_stats) return fail(LINETR_E_ARG, "describe_ragged: a training-mode handle (bn_batch_stats = 1) runs linetr_forward_train only");
  if (int e = check_cu(h_cu, n_images)) return e;
  if (h_cu[n_images] != N) return fail(LINETR_E_ARG, "describe_ragged: cu_sub does not end at N");
  MapFormat mf;
  if (int e = check_images(h_images, n_images, dense_is_nhwc, mf)) return e;
  if (K <= 0 || N <= 0) return LINETR_OK;
  if (!d_recs || !d_line_desc || !d_ws) return fail(LINETR_E_ARG, "describe_ragged: null pointer");
  if (T < 1 || T > 4096) return fail(LINETR_E_ARG, "describe_ragged: bad max_tokens");
  if (n_real < N || n_real > (int64_t)N * T) return fail(LINETR_E_ARG, "describe_ragged: implausible real-token count");
  if (out.desc && !out.pnt) return fail(LINETR_E_ARG, "describe_ragged: out.desc requires out.pnt");
  if (!aligned16(out.desc) || !aligned16(d_ws))
    return fail(LINETR_E_ARG, "describe_ragged: out.desc and the workspace must be 16-byte aligned");
  // the kernels index the table with the records' image: with the host copy of the records at hand, every one is looked at first
  for (int k = 0; h_recs && k < K; ++k)
    if (h_recs[k].image < 0 || h_recs[k].image >= n_images)
      return fail(LINETR_E_ARG, "describe_ragged: record %d belongs to image %d, outside the table of %d", k, h_recs[k].image, n_images);
  K2sTable k2s;
  if (int e = k2s_table(out, n_images, K, N, h_cu, k2s, "describe_ragged")) return e;
  if (ws_bytes < describe_ragged_total(h, h_images, n_images, mf, N, n_real))   // (a saturated total refuses every workspace)
    return fail(LINETR_E_WORKSPACE, "describe_ragged: workspace too small");
  const int64_t rows = n_real + n_images;
  if (rows > INT32_MAX / 8) return fail(LINETR_E_ARG, "describe_ragged: batch too large");
  LT_HIP(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  // the image table: made in a pinned staging slot (the caller's array is not read after this call), one asynchronous copy
  int slot = -1;
  RaggedImage* tab = (RaggedImage*)staging_ring().acquire((size_t)n_images * sizeof(RaggedImage), &slot);
  if (!tab) return fail(LINETR_E_HIP, "describe_ragged: pinned staging allocation failed");
  const RaggedFront rf = ragged_front(h_images, n_images, mf, (char*)d_ws, tab);
  RaggedImage* d_tab = (RaggedImage*)((char*)d_ws + rf.o_tab);
  LT_HIP(hipMemcpyAsync(d_tab, tab, (size_t)n_images * sizeof(RaggedImage), hipMemcpyHostToDevice, st));
  if (int e = staging_ring().commit(slot, st)) return e;
  char* rest = (char*)d_ws + rf.total;
  DescWs dw = desc_layout(0, 0, 0, N, rows, rest);
  TokenFront f{d_recs, K, N, 0.0, T, nullptr, nullptr, n_images, 0, 0, align_corners, mf, 0.0, 0.0};
  f.tab = d_tab; f.max_cells = rf.max_cells; f.cells = rf.cells;
  return describe_launch(h, st, f, dw, rest + dw.fwd_off, out, k2s, d_sub2line, d_line_desc, h_cu, d_cu, n_real, nullptr);
}

namespace {

// the streams and events of the describe pipeline, made at the first submit: all or nothing
int pipe_ready(LinetrHandle* h) {
  LinetrHandle::Pipe& p = h->pipe;
  if (p.stream[0]) return LINETR_OK;
  if (p.failed) return fail(LINETR_E_HIP, "describe_submit: the pipeline's streams could not be created");
  constexpr int NS = LinetrHandle::PIPE_STREAMS, NL = LinetrHandle::PIPE_SLOTS, NE = NL * (NS + 1);
  hipStream_t s[NS] = {};
  hipEvent_t ev[NE] = {};
  bool ok = true;
  for (int i = 0; ok && i < NS; ++i) ok = hipStreamCreateWithFlags(&s[i], hipStreamNonBlocking) == hipSuccess;
  for (int i = 0; ok && i < NE; ++i) ok = hipEventCreateWithFlags(&ev[i], hipEventDisableTiming) == hipSuccess;
  if (!ok) {
    for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
    for (hipStream_t x : s) if (x) (void)hipStreamDestroy(x);
    (void)hipGetLastError();
    p.failed = true;
    return fail(LINETR_E_HIP, "describe_submit: the pipeline's streams could not be created");
  }
  for (int i = 0; i < NS; ++i) p.stream[i] = s[i];
  for (int l = 0, k = 0; l < NL; ++l) {
    p.fork[l] = ev[k++]; p.done[l] = ev[k++];
    for (int c = 0; c < NS - 1; ++c) p.cut[l][c] = ev[k++];
  }
  return LINETR_OK;
}

// How a batch is cut into stages when the caller keeps `n_slots` batches in flight.
struct PipePlan { int n_cuts = 0; int cut[LinetrHandle::PIPE_STREAMS - 1] = {0, 0, 0}; };
PipePlan pipe_plan(const LinetrHandle* h, int n_slots) {
  PipePlan pl;
  // measured on MI355X (profiles/r06_pipeline_sweep.txt): balanced stages win over "front | signature network" (the front is a third
  // of a batch), and three stages over two; a fourth slot only lets the host run one more batch ahead
  const int n_sig = (int)h->sig.size();
  if (n_slots == 2 || n_sig < 5) { pl.n_cuts = 1; pl.cut[0] = n_sig >= 3 ? CUT_SIG0 + 2 : CUT_SENTENCE; }
  else { pl.n_cuts = 2; pl.cut[0] = CUT_SIG0; pl.cut[1] = CUT_SIG0 + 3; }
  return pl;
}
}  // namespace

extern "C" int linetr_describe(LinetrHandle* h, const LinetrLineRec* d_recs, int32_t K, int32_t N, int64_t n_real,
                               const int32_t* h_cu, const int32_t* d_cu, int32_t n_images, double td, int32_t T,
                               const void* d_dense_desc, const float* d_dense_score, int32_t height, int32_t width,
                               int32_t align_corners, int32_t dense_is_nhwc, LinetrTokens out, int32_t* d_sub2line,
                               float* d_line_desc, void* d_ws, int64_t ws_bytes, void* stream) {
  return describe_impl(h, d_recs, K, N, n_real, h_cu, d_cu, n_images, td, T, d_dense_desc, d_dense_score, height, width, align_corners,
                       dense_is_nhwc, out, d_sub2line, d_line_desc, d_ws, ws_bytes, (hipStream_t)stream, nullptr);
}

extern "C" int32_t linetr_pipeline_max_slots(void) { return LinetrHandle::PIPE_SLOTS; }

extern "C" int linetr_describe_submit(LinetrHandle* h, const LinetrLineRec* d_recs, int32_t K, int32_t N, int64_t n_real,
                                      const int32_t* h_cu, const int32_t* d_cu, int32_t n_images, double td, int32_t T,
                                      const void* d_dense_desc, const float* d_dense_score, int32_t height, int32_t width,
                                      int32_t align_corners, int32_t dense_is_nhwc, LinetrTokens out, int32_t* d_sub2line,
                                      float* d_line_desc, void* d_ws, int64_t ws_bytes, int32_t slot, int32_t n_slots, void* stream) {
  if (!h) return fail(LINETR_E_ARG, "describe_submit: null handle");
  if (n_slots < 1 || n_slots > LinetrHandle::PIPE_SLOTS || slot < 0 || slot >= n_slots)
    return fail(LINETR_E_ARG, "describe_submit: need 0 <= slot < n_slots <= %d", LinetrHandle::PIPE_SLOTS);
  LT_HIP(hipSetDevice(h->device));
  if (int e = pipe_ready(h)) return e;
  LinetrHandle::Pipe& p = h->pipe;
  hipStream_t st = (hipStream_t)stream;
  // host run-ahead is bounded to the batches in flight: the slot's previous batch (n_slots submits ago) must have left the GPU
  // before its workspace is handed to the device again
  if (p.submitted[slot]) LT_HIP(hipEventSynchronize(p.done[slot]));
  const PipePlan plan = pipe_plan(h, n_slots);
  PipeStages stg;
  for (int i = 0; i < LinetrHandle::PIPE_STREAMS; ++i) stg.stream[i] = p.stream[i];
  stg.n_cuts = plan.n_cuts;
  for (int i = 0; i < plan.n_cuts; ++i) { stg.cut[i] = plan.cut[i]; stg.ev[i] = p.cut[slot][i]; }
  // fork: the first stage starts behind everything the caller has queued so far (the upload of d_recs, the producer of the maps)
  LT_HIP(hipEventRecord(p.fork[slot], st));
  LT_HIP(hipStreamWaitEvent(stg.stream[0], p.fork[slot], 0));
  const int e = describe_impl(h, d_recs, K, N, n_real, h_cu, d_cu, n_images, td, T, d_dense_desc, d_dense_score, height, width,
                              align_corners, dense_is_nhwc, out, d_sub2line, d_line_desc, d_ws, ws_bytes, stg.stream[0], &stg);
  if (e) {   // leave the streams idle and the slot free: a failed submit must not leave half a batch behind
    for (hipStream_t x : p.stream) (void)hipStreamSynchronize(x);
    p.submitted[slot] = false;
    return e;
  }
  // the stream of the last stage reached (an empty batch queues nothing: the event then completes with what that stream already holds)
  LT_HIP(hipEventRecord(p.done[slot], stg.stream[stg.next]));
  p.submitted[slot] = true;
  return LINETR_OK;
}

extern "C" int linetr_describe_join(LinetrHandle* h, int32_t slot, void* stream) {
  if (!h) return fail(LINETR_E_ARG, "describe_join: null handle");
  if (slot < 0 || slot >= LinetrHandle::PIPE_SLOTS) return fail(LINETR_E_ARG, "describe_join: bad slot");
  if (!h->pipe.stream[0] || !h->pipe.submitted[slot]) return fail(LINETR_E_ARG, "describe_join: nothing was submitted to this slot");
  LT_HIP(hipStreamWaitEvent((hipStream_t)stream, h->pipe.done[slot], 0));
  return LINETR_OK;
}

extern "C" int linetr_debug_posenc(LinetrHandle* h, int32_t which, const float* d_in0, const float* d_in1,
                                      const float* d_in2, int64_t rows, float* d_out, void* stream) {
  if (!h || !d_in0 || !d_in1 || !d_out || (which == 1 && !d_in2) || which < 0 || which > 1)
    return fail(LINETR_E_ARG, "debug_posenc: bad argument");
  if (!fused_mlp_enabled(h->cfg)) return fail(LINETR_E_ARG, "debug_posenc: needs keyline_encoder [32,64,128,256]");
  if (rows <= 0) return LINETR_OK;
  LT_HIP(hipSetDevice(h->device));
  return enc_mlp123(h, (hipStream_t)stream, EncCall{which, d_in0, d_in1, which == ENC_WORD ? nullptr : d_in2, rows, nullptr}, d_out);
}

extern "C" int linetr_debug_gemm(LinetrHandle* h, const float* A, int32_t lda, const float* W, const float* bias,
                                 const float* R, float* Y, int32_t ldy, int32_t M, int32_t N, int32_t K, int32_t act,
                                 int32_t cache_weights, void* stream) {
  if (lda < K || ldy < N || lda % 4 || ldy % 4) return fail(LINETR_E_ARG, "debug_gemm: bad leading dimension");
  if (!h || !A || !W || !Y) return fail(LINETR_E_ARG, "debug_gemm: null argument");
  if (K % 32 || N % 64) return fail(LINETR_E_ARG, "debug_gemm: N %% 64 == 0 and K %% 32 == 0 required");
  LT_HIP(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  GemmW w;
  w.W = W; w.b = bias; w.rows = N; w.K = K;
  unsigned char* buf = nullptr;   // this call's own scratch buffer (not cached), freed below
  if (h->precision != LINETR_PREC_F32) {
    // caller-provided weights: their split copies in a scratch buffer (optionally cached by pointer); the weight-stationary
    // kernel's shape also reads a split-tile image
    int64_t bytes = 0;
    const SplitOffsets at = split_offsets(N, K, N == WS_N && K == WS_K, bytes);
    auto it = h->debug_split.find(W);
    const bool make = it == h->debug_split.end();
    if (make) LT_HIP(hipMalloc((void**)&buf, bytes));
    split_copies(w, make ? buf : it->second, at, make, st);
    LT_LAUNCH_CHECK();
    if (make && cache_weights) { h->debug_split[W] = buf; buf = nullptr; }
  }
  const int e = run_gemm(h, st, w, M, {A, lda}, {Y, ldy}, act, R);
  if (buf) {
    (void)hipStreamSynchronize(st);
    (void)hipFree(buf);
  }
  return e;
}

extern "C" int linetr_debug_gemm_case(LinetrHandle* h, const LinetrGemmCase* c, int32_t* tile_used, void* stream) {
  if (!h || !c) return fail(LINETR_E_ARG, "debug_gemm_case: null argument");
  const bool query = !c->A && !c->W && !c->Y;     // nothing is dereferenced: A2 / R only say that the operand is there
  const int M = c->M, N = c->N, K = c->K, groups = c->groups;
  if (M < 0 || N <= 0 || K <= 0 || groups < 1) return fail(LINETR_E_ARG, "debug_gemm_case: bad shape M=%d N=%d K=%d groups=%d", M, N, K, groups);
  if (K % 32 || N % 64) return fail(LINETR_E_ARG, "debug_gemm_case: N %% 64 == 0 and K %% 32 == 0 required");
  if (c->lda % 4 || c->ldy % 4 || c->ldy < N || (c->A2 && (c->lda2 % 4 || c->lda2 < K - c->K1)) || c->lda < (c->A2 ? c->K1 : K))
    return fail(LINETR_E_ARG, "debug_gemm_case: bad leading dimension");
  if (c->A2 && (c->K1 <= 0 || c->K1 >= K || c->K1 % 32))
    return fail(LINETR_E_ARG, "debug_gemm_case: the split point K1 = %d must be a multiple of 32 inside (0, K = %d)", c->K1, K);
  if (c->gA % 4 || c->gY % 4 || c->gA < 0 || c->gY < 0) return fail(LINETR_E_ARG, "debug_gemm_case: group strides must be non-negative multiples of 4 floats");
  if (c->act < ACT_NONE || c->act > ACT_DIST) return fail(LINETR_E_ARG, "debug_gemm_case: act must be 0 .. 3");
  if (c->tile < -1 || (c->tile >= (int)SplitTile::count && c->tile != LINETR_GEMM_TILE_WS))
    return fail(LINETR_E_ARG, "debug_gemm_case: no tile %d", c->tile);
  NormSpec ns;
  if (c->norm) {
    if (c->norm != 1 && c->norm != 2) return fail(LINETR_E_ARG, "debug_gemm_case: norm must be 0, 1 (LayerNorm) or 2 (L2)");
    if (N != D || c->ldy != D || groups != 1) return fail(LINETR_E_ARG, "debug_gemm_case: a row normalisation needs N = ldy = 256 and one group");
    if (!query && c->norm == 1 && (!c->gamma || !c->beta)) return fail(LINETR_E_ARG, "debug_gemm_case: LayerNorm needs gamma and beta");
    ns.mode = c->norm; ns.gamma = c->gamma; ns.beta = c->beta; ns.add2 = c->add2; ns.eps = c->eps;
  } else if (c->via_row_norm) {
    return fail(LINETR_E_ARG, "debug_gemm_case: via_row_norm without a norm");
  }
  if (!query) {
    if (!c->A || !c->W || !c->Y) return fail(LINETR_E_ARG, "debug_gemm_case: null tensor");
    uintptr_t al = (uintptr_t)c->A | (uintptr_t)c->A2 | (uintptr_t)c->W | (uintptr_t)c->bias | (uintptr_t)c->R | (uintptr_t)c->Y |
                   (uintptr_t)c->gamma | (uintptr_t)c->beta | (uintptr_t)c->add2;
    if (al % 16) return fail(LINETR_E_ARG, "debug_gemm_case: tensors must be 16-byte aligned");
  }
  const int64_t rows = (int64_t)N * groups;
  const bool with_st = groups == 1 && N == WS_N && K == WS_K;
  GemmW w;
  w.W = c->W; w.b = c->bias; w.rows = (int)rows; w.K = K;
  const GemmA A{c->A, c->lda, c->A2, c->lda2, c->A2 ? c->K1 : 0};
  const GemmGroups grp{groups, N, c->gA, c->gY};
  const GemmGroups* pg = groups > 1 ? &grp : nullptr;
  GemmForce force;
  force.tile = c->tile; force.used = tile_used; force.launch = false;
  // a forced tile normalises in its epilogue or is refused; the dispatcher's choice falls back to row_norm_kernel as run_gemm_norm does
  const bool fuse = c->norm && !c->via_row_norm && (c->tile >= 0 || gemm_norm_fuses(h, w, M, A, c->R, c->Y));
  // first pass: the choice and every refusal, nothing launched
  if (with_st) w.st = reinterpret_cast<const unsigned char*>(h);   // only its presence is read; split_copies makes the image below
  if (int e = run_gemm(h, nullptr, w, M, A, {c->Y, c->ldy}, c->act, c->R, pg, fuse ? &ns : nullptr, &force)) return e;
  if (query || M == 0) return LINETR_OK;
  LT_HIP(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  unsigned char* buf = nullptr;   // this call's scratch: the split copies of W and, for row_norm_kernel, the un-normalised product
  int64_t bytes = 0;
  SplitOffsets at{};
  if (h->precision != LINETR_PREC_F32) at = split_offsets(rows, K, with_st, bytes);
  bytes = align_up(bytes, 256);
  const int64_t tmp_at = bytes;
  if (c->norm && !fuse) bytes += (int64_t)M * D * sizeof(float);
  if (bytes > 0) LT_HIP(hipMalloc((void**)&buf, bytes));
  if (h->precision != LINETR_PREC_F32) split_copies(w, buf, at, true, st);
  int e = LINETR_OK;
  if (hipGetLastError() != hipSuccess) e = fail(LINETR_E_HIP, "debug_gemm_case: splitting the weights failed");
  force.launch = true;
  if (!e && c->norm && !fuse) {
    float* tmp = reinterpret_cast<float*>(buf + tmp_at);
    e = run_gemm(h, st, w, M, A, {tmp, D}, c->act, c->R, nullptr, nullptr, &force);
    if (!e) e = row_norm(h, st, tmp, M, ns, c->Y);
  } else if (!e) {
    e = run_gemm(h, st, w, M, A, {c->Y, c->ldy}, c->act, c->R, pg, fuse ? &ns : nullptr, &force);
  }
  (void)hipStreamSynchronize(st);
  if (buf) (void)hipFree(buf);
  return e;
}

extern "C" int linetr_debug_sig_attention(LinetrHandle* h, int32_t kernel, int32_t layer, const float* d_in, int32_t ld_in,
                                          const int32_t* h_cu, int32_t n_images, float* d_msg, int32_t* kernel_used, void* stream) {
  if (!h) return fail(LINETR_E_ARG, "debug_sig_attention: null handle");
  if (h->cfg.bn_batch_stats) return fail(LINETR_E_ARG, "debug_sig_attention: a training-mode handle (bn_batch_stats = 1) is not served");
  const bool eight_waves = kernel == (SIGK_FUSED | LINETR_SIG_EIGHT_WAVES);
  if (eight_waves) kernel = SIGK_FUSED;
  if (kernel < -1 || kernel > SIGK_FUSED)
    return fail(LINETR_E_ARG, "debug_sig_attention: kernel must be -1 .. 4 (or 4 + %d: eight compute waves)", LINETR_SIG_EIGHT_WAVES);
  if (int e = check_cu(h_cu, n_images)) return e;
  const int N = h_cu[n_images];
  int max_n = 0;
  for (int i = 0; i < n_images; ++i) max_n = std::max(max_n, h_cu[i + 1] - h_cu[i]);
  const bool query_only = kernel == -1 && !d_in && !d_msg;
  if (kernel == -1) kernel = sig_attn_plan(h, n_images, N, max_n).kernel();
  if (kernel_used) *kernel_used = kernel | (eight_waves ? LINETR_SIG_EIGHT_WAVES : 0);
  if (query_only) return LINETR_OK;
  // what a kernel is not written for is refused, not launched
  if (kernel == SIGK_FUSED) {
    if (h->precision != LINETR_PREC_BF16X6) return fail(LINETR_E_ARG, "debug_sig_attention: the fused kernel runs in bf16x6 mode only");
    if (max_n > 256) return fail(LINETR_E_ARG, "debug_sig_attention: the fused kernel takes images of up to 256 sub-lines");
    if (layer < 0 || layer >= (int)h->sig.size()) return fail(LINETR_E_ARG, "debug_sig_attention: layer out of range");
    if (!h->sig[layer].Wqkv.st) return fail(LINETR_E_ARG, "debug_sig_attention: the layer has no split-tile weight image");
    if (ld_in != D) return fail(LINETR_E_ARG, "debug_sig_attention: the fused kernel reads z rows, ld_in must be 256");
  } else if (ld_in != 3 * D && !(kernel == SIGK_SMALL && ld_in == 4 * D)) {
    return fail(LINETR_E_ARG, "debug_sig_attention: ld_in must be 768 (or 1024, sig_attn_small only)");
  }
  if (N <= 0) return LINETR_OK;
  if (!d_in || !d_msg) return fail(LINETR_E_ARG, "debug_sig_attention: null tensor");
  if (((uintptr_t)d_in | (uintptr_t)d_msg) % 16) return fail(LINETR_E_ARG, "debug_sig_attention: tensors must be 16-byte aligned");
  LT_HIP(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  int* cu_dev = nullptr;
  LT_HIP(hipMalloc((void**)&cu_dev, (n_images + 1) * sizeof(int)));
  int e = LINETR_OK;
  if (hipMemcpyAsync(cu_dev, h_cu, (n_images + 1) * sizeof(int), hipMemcpyHostToDevice, st) != hipSuccess)
    e = fail(LINETR_E_HIP, "debug_sig_attention: cu_sub upload failed");
  const double fl = attn_flops(h_cu, n_images);
  if (!e)
    e = kernel == SIGK_FUSED ? sig_qkv_attention(h, st, h->sig[layer], d_in, cu_dev, n_images, N, max_n, eight_waves, fl, d_msg)
                             : sig_attention(h, st, kernel, d_in, ld_in, cu_dev, n_images, N, max_n, fl, d_msg);
  (void)hipStreamSynchronize(st);
  (void)hipFree(cu_dev);
  return e;
}

extern "C" int linetr_debug_tok_mlp(LinetrHandle* h, int32_t variant, const float* d_pnt, const float* d_score, int64_t rows_word,
                                    const float* d_sublines, const float* d_resp, const float* d_angle, int64_t rows_line,
                                    float* d_out_word, float* d_out_line, int32_t max_blocks, int32_t* variant_used, void* stream) {
  if (!h) return fail(LINETR_E_ARG, "debug_tok_mlp: null handle");
  if (h->cfg.bn_batch_stats) return fail(LINETR_E_ARG, "debug_tok_mlp: a training-mode handle (bn_batch_stats = 1) is not served");
  if (variant < -1 || variant > TOKV_CHAIN) return fail(LINETR_E_ARG, "debug_tok_mlp: variant must be -1 .. 4");
  if (rows_word < 0 || rows_line < 0 || rows_word > INT32_MAX / 8 || rows_line > INT32_MAX / 8)
    return fail(LINETR_E_ARG, "debug_tok_mlp: row counts must be 0 .. %d", INT32_MAX / 8);
  if (max_blocks < 0) return fail(LINETR_E_ARG, "debug_tok_mlp: max_blocks must be 0 (one block per compute unit) or positive");
  if (!fused_mlp_enabled(h->cfg) || h->cfg.enc_channels[0] != 32 || h->cfg.enc_channels[3] != D)
    return fail(LINETR_E_ARG, "debug_tok_mlp: needs keyline_encoder [32,64,128,256]");
  const bool query_only = variant == -1 && !d_out_word && !d_out_line;
  // which encoders run: the forced single-encoder variants their own, everything else every encoder that has rows
  bool word = rows_word > 0 && variant != TOKV_LINE, line = rows_line > 0 && variant != TOKV_WORD;
  if (variant == -1) {
    const TokMlpPlan plan = tok_mlp_plan(h, rows_word, rows_line);
    variant = plan.both >= 0 ? plan.both : (word && !plan.word) || (line && !plan.line) ? (int)TOKV_CHAIN : word ? (int)TOKV_WORD : line ? (int)TOKV_LINE : -1;
  }
  if (variant_used) *variant_used = variant;
  if (query_only || variant < 0) return LINETR_OK;
  // what a launch is not written for is refused, not launched
  if (variant == TOKV_DUAL || variant == TOKV_SEQ) {
    if (rows_word <= 0 || rows_line <= 0) return fail(LINETR_E_ARG, "debug_tok_mlp: the two-encoder launches need rows of both encoders");
    if (variant == TOKV_DUAL && !tok_mlp_dual_fits(rows_word, rows_line))
      return fail(LINETR_E_ARG, "debug_tok_mlp: %lld + %lld rows do not fit the chip side by side (one block per 64-row tile, %d compute units)",
                  (long long)rows_word, (long long)rows_line, cu_count());
  }
  if (variant != TOKV_CHAIN && ((word && !tok_mlp_has_images(h->enc[ENC_WORD])) || (line && !tok_mlp_has_images(h->enc[ENC_LINE]))))
    return fail(LINETR_E_ARG, "debug_tok_mlp: the encoder has no split-tile weight images");
  if (!word && !line) return LINETR_OK;
  if ((word && (!d_pnt || !d_score || !d_out_word)) || (line && (!d_sublines || !d_resp || !d_angle || !d_out_line)))
    return fail(LINETR_E_ARG, "debug_tok_mlp: null tensor");
  if (((uintptr_t)d_pnt | (uintptr_t)d_score | (uintptr_t)d_sublines | (uintptr_t)d_resp | (uintptr_t)d_angle) % 4 ||
      ((uintptr_t)d_out_word | (uintptr_t)d_out_line) % 16)
    return fail(LINETR_E_ARG, "debug_tok_mlp: outputs must be 16-byte aligned, inputs 4-byte aligned");
  LT_HIP(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  float* scratch = nullptr;   // the unfused chain's [rows][128] activations, freed below
  const int64_t off_line = align_up((word ? rows_word : 0) * h->cfg.enc_channels[2] * 4, 256);
  if (variant == TOKV_CHAIN) LT_HIP(hipMalloc((void**)&scratch, off_line + align_up((line ? rows_line : 0) * h->cfg.enc_channels[2] * 4, 256) + 256));
  float* act_w[4] = {nullptr, nullptr, scratch, d_out_word};
  float* act_l[4] = {nullptr, nullptr, scratch ? (float*)((char*)scratch + off_line) : nullptr, d_out_line};
  const EncCall cw{ENC_WORD, d_pnt, d_score, nullptr, rows_word, act_w};
  const EncCall cl{ENC_LINE, d_sublines, d_resp, d_angle, rows_line, act_l};
  int e = LINETR_OK;
  switch (variant) {
    case TOKV_WORD: e = tok_mlp_launch(tok_mlp_args(h, cw), true, st, max_blocks); break;
    case TOKV_LINE: e = tok_mlp_launch(tok_mlp_args(h, cl), false, st, max_blocks); break;
    case TOKV_DUAL: e = tok_mlp_launch_dual(tok_mlp_args(h, cw), tok_mlp_args(h, cl), st, max_blocks, 0); break;
    case TOKV_SEQ: e = tok_mlp_launch_dual(tok_mlp_args(h, cw), tok_mlp_args(h, cl), st, max_blocks, 1); break;
    default:
      if (word) e = pos_encoder(h, st, cw, false);
      if (!e && line) e = pos_encoder(h, st, cl, false);
  }
  (void)hipStreamSynchronize(st);
  if (scratch) (void)hipFree(scratch);
  return e;
}

namespace {
// linetr_debug_bn_train's workspace: [the chain's act[0 .. 2] |] partial | affine
constexpr int64_t BN_PARTIAL_BYTES = (int64_t)BN_MAX_BLOCKS * 2 * BN_MAX_CHANNELS * 8, BN_AFFINE_BYTES = 2 * BN_MAX_CHANNELS * 4;
struct BnDebugWs { float* act[3]; double* partial; float* affine; int64_t total; };
BnDebugWs bn_debug_layout(const LinetrHandle* h, int which, int64_t rows, char* base) {
  BnDebugWs w;
  int64_t off = 0;
  auto take = [&](int64_t bytes) { char* p = base + off; off += align_up(bytes, 256); return p; };
  for (int i = 0; i < 3; ++i) w.act[i] = (float*)take(which < 0 ? 0 : std::max<int64_t>(rows, 0) * h->cfg.enc_channels[i] * 4);
  w.partial = (double*)take(BN_PARTIAL_BYTES);
  w.affine = (float*)take(BN_AFFINE_BYTES);
  w.total = off;
  return w;
}
}  // namespace

extern "C" int64_t linetr_debug_bn_train_workspace_bytes(const LinetrHandle* h, int32_t which, int64_t rows) {
  if (!h || which < -1 || which > 1 || rows < 0 || rows > INT32_MAX / 8) return -1;
  return bn_debug_layout(h, which, rows, nullptr).total;
}

extern "C" int linetr_debug_bn_train(LinetrHandle* h, int32_t which, float* d_z, int64_t rows, int32_t C, int32_t ld,
                                     const float* d_gamma, const float* d_beta, const float* d_in0, const float* d_in1,
                                     const float* d_in2, float* d_out, float momentum, float* d_running, float* d_batch,
                                     float* d_affine, int32_t* nb_used, void* d_ws, int64_t ws_bytes, void* stream) {
  if (!h) return fail(LINETR_E_ARG, "debug_bn_train: null handle");
  if (!h->cfg.bn_batch_stats) return fail(LINETR_E_ARG, "debug_bn_train: the handle was created for inference (bn_batch_stats = 0)");
  if (which < -1 || which > 1) return fail(LINETR_E_ARG, "debug_bn_train: which must be -1 (one layer), 0 (word encoder) or 1 (line encoder)");
  if (rows < 0 || rows > INT32_MAX / 8) return fail(LINETR_E_ARG, "debug_bn_train: row count must be 0 .. %d", INT32_MAX / 8);
  if (!(momentum >= 0.f && momentum <= 1.f)) return fail(LINETR_E_ARG, "debug_bn_train: momentum out of [0, 1]");
  if (nb_used) *nb_used = 0;
  if (which < 0) {
    // (bn_train_layer has these checks too; here they come before anything else is looked at)
    if (!bn_channels_ok(C)) return fail(LINETR_E_ARG, "debug_bn_train: %d channels (4 .. %d, multiples of 4)", C, BN_MAX_CHANNELS);
    if (!bn_rows_ok(d_z, ld, C))
      return fail(LINETR_E_ARG, "debug_bn_train: row stride %d (at least the %d channels, a multiple of 4) on a 16-byte aligned z", ld, C);
    if (!d_z || !d_gamma || !d_beta || !d_running) return fail(LINETR_E_ARG, "debug_bn_train: null tensor");
    if (((uintptr_t)d_gamma | (uintptr_t)d_beta | (uintptr_t)d_running | (uintptr_t)d_batch | (uintptr_t)d_affine) % 4)
      return fail(LINETR_E_ARG, "debug_bn_train: the vectors must be 4-byte aligned");
  } else {
    if (!d_in0 || !d_in1 || (which == ENC_LINE && !d_in2) || !d_out || !d_running) return fail(LINETR_E_ARG, "debug_bn_train: null tensor");
    if (((uintptr_t)d_in0 | (uintptr_t)d_in1 | (uintptr_t)d_in2 | (uintptr_t)d_running | (uintptr_t)d_batch) % 4 || (uintptr_t)d_out % 16)
      return fail(LINETR_E_ARG, "debug_bn_train: the output must be 16-byte aligned, the other tensors 4-byte aligned");
  }
  if (!d_ws || (uintptr_t)d_ws % 256) return fail(LINETR_E_ARG, "debug_bn_train: the workspace must be 256-byte aligned");
  const BnDebugWs w = bn_debug_layout(h, which, rows, (char*)d_ws);
  if (ws_bytes < w.total) return fail(LINETR_E_WORKSPACE, "debug_bn_train: workspace too small (%lld < %lld bytes)", (long long)ws_bytes, (long long)w.total);
  if (rows == 0) return LINETR_OK;
  LT_HIP(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  BnTrain bt;
  bt.running = d_running; bt.batch = d_batch; bt.momentum = momentum; bt.partial = w.partial; bt.affine = w.affine;
  int e, nb = 0;
  if (which < 0) {
    e = bn_train_layer(st, bt, d_z, rows, C, ld, d_gamma, d_beta, 0, &nb);
    if (!e && d_affine && hipMemcpyAsync(d_affine, w.affine, (size_t)2 * C * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess)
      e = fail(LINETR_E_HIP, "debug_bn_train: copying alpha | beta' failed");
  } else {
    float* act[4] = {w.act[0], w.act[1], w.act[2], d_out};
    const EncCall c{which, d_in0, d_in1, d_in2, rows, act};
    int64_t off = 0;
    e = pos_encoder_bn(h, st, c, bt, off);
    nb = bn_row_chunks(rows);
  }
  if (nb_used) *nb_used = nb;
  (void)hipStreamSynchronize(st);
  return e;
}

extern "C" int linetr_debug_cls_pool(LinetrHandle* h, int32_t kernel, const LinetrLineRec* d_recs, int32_t K, const int32_t* d_sub2line,
                                     int32_t N, int32_t T, const float* d_cpnt, const float* d_a4, int64_t first_pad, int32_t n_images,
                                     const void* d_map, int32_t dense_is_nhwc, int32_t Hc, int32_t Wc, int32_t align_corners,
                                     const float* d_desc_dense, float* d_pooled, int32_t* kernel_used, void* stream) {
  if (!h) return fail(LINETR_E_ARG, "debug_cls_pool: null handle");
  if (h->cfg.bn_batch_stats) return fail(LINETR_E_ARG, "debug_cls_pool: a training-mode handle (bn_batch_stats = 1) is not served");
  if (kernel < -1 || kernel > POOLK_SPLIT4) return fail(LINETR_E_ARG, "debug_cls_pool: kernel must be -1 .. 3");
  if (N < 0) return fail(LINETR_E_ARG, "debug_cls_pool: negative sub-line count");
  if (kernel == -1) kernel = cls_pool_plan(d_desc_dense == nullptr, N);   // d_desc_dense says that the token stage is the dense one
  if (kernel_used) *kernel_used = kernel;
  if (!d_pooled) return LINETR_OK;                                         // the choice only: nothing is dereferenced
  if (T < 1 || T > 4096) return fail(LINETR_E_ARG, "debug_cls_pool: max_tokens must be 1 .. 4096");
  if (N == 0) return LINETR_OK;
  if (!d_a4) return fail(LINETR_E_ARG, "debug_cls_pool: null tensor");
  if (((uintptr_t)d_a4 | (uintptr_t)d_pooled) % 16) return fail(LINETR_E_ARG, "debug_cls_pool: tensors must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  TokenStage ts;
  if (kernel == POOLK_DENSE) {
    if (!d_desc_dense || (uintptr_t)d_desc_dense % 16) return fail(LINETR_E_ARG, "debug_cls_pool: the dense kernel reads d_desc_dense [N][T][256], 16-byte aligned");
    if ((int64_t)N * T > INT32_MAX / 8) return fail(LINETR_E_ARG, "debug_cls_pool: batch too large");
    LT_HIP(hipSetDevice(h->device));
    ts.desc = d_desc_dense; ts.rows = (int64_t)N * T;
    const int e = cls_pool_launch(h, st, kernel, ts, 1, N, T, d_a4, d_pooled);
    (void)hipStreamSynchronize(st);
    return e;
  }
  if (!d_recs || !d_sub2line || !d_cpnt || !d_map) return fail(LINETR_E_ARG, "debug_cls_pool: null tensor");
  if (K < 1 || n_images < 1 || Hc < 1 || Wc < 1 || first_pad < 0 || first_pad > INT32_MAX / 8 || (int64_t)n_images * Hc * Wc > INT32_MAX / D)
    return fail(LINETR_E_ARG, "debug_cls_pool: bad shape");
  MapFormat mf;
  if (int e = map_format(dense_is_nhwc, "debug_cls_pool", mf)) return e;
  if ((uintptr_t)d_recs % 8 || ((uintptr_t)d_sub2line | (uintptr_t)d_cpnt) % 4 || !mf.aligned(d_map) || (mf.type == MT_F32 && (uintptr_t)d_map % 4))
    return fail(LINETR_E_ARG, "debug_cls_pool: misaligned tensor (records 8 bytes, an NHWC map 16 (half: 8), an NCHW map its element, the others 4)");
  LT_HIP(hipSetDevice(h->device));
  {  // everything the kernel indexes with comes from the caller: checked on the host first
    std::vector<LinetrLineRec> recs(K);
    std::vector<int32_t> s2l(N);
    LT_HIP(hipStreamSynchronize(st));
    LT_HIP(hipMemcpy(recs.data(), d_recs, (size_t)K * sizeof(LinetrLineRec), hipMemcpyDeviceToHost));
    LT_HIP(hipMemcpy(s2l.data(), d_sub2line, (size_t)N * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (int n = 0; n < N; ++n) {
      if (s2l[n] < 0 || s2l[n] >= K) return fail(LINETR_E_ARG, "debug_cls_pool: sub-line %d maps to key-line %d, outside [0, %d)", n, s2l[n], K);
      const LinetrLineRec& r = recs[s2l[n]];
      const int64_t j = (int64_t)n - r.first_sub;
      if (j < 0 || j >= r.n_sub || j * T >= r.n_tok)
        return fail(LINETR_E_ARG, "debug_cls_pool: sub-line %d is not one of key-line %d's (first_sub %d, n_sub %d, n_tok %d)", n, s2l[n], r.first_sub, r.n_sub, r.n_tok);
      if (r.first_tok < 0 || (int64_t)r.first_tok + r.n_tok > first_pad)
        return fail(LINETR_E_ARG, "debug_cls_pool: key-line %d's tokens [%d, %d + %d) reach past first_pad = %lld", s2l[n], r.first_tok, r.first_tok, r.n_tok, (long long)first_pad);
      if (r.image < 0 || r.image >= n_images) return fail(LINETR_E_ARG, "debug_cls_pool: key-line %d's image %d outside [0, %d)", s2l[n], r.image, n_images);
    }
  }
  void* buf = nullptr;   // the transposed map of an NCHW caller, freed below
  if (!mf.nhwc) LT_HIP(hipMalloc(&buf, (size_t)n_images * Hc * Wc * D * mf.esize));
  ts.cpnt = d_cpnt; ts.recs = d_recs; ts.sub2line_g = d_sub2line; ts.rows = first_pad + n_images; ts.first_pad = first_pad;
  ts.Hc = Hc; ts.Wc = Wc; ts.align_corners = align_corners;
  ts.map_type = mf.type;
  int e = nhwc_map(h, st, d_map, mf, n_images, Hc * Wc, buf, ts.nhwc);
  if (!e) e = cls_pool_launch(h, st, kernel, ts, n_images, N, T, d_a4, d_pooled);
  (void)hipStreamSynchronize(st);
  if (buf) (void)hipFree(buf);
  return e;
}

// One stage of forward_core alone on the caller's rows: the same host functions, the handle's weights, forward_core's own workspace
// layout (no token rows).  Everything is checked before the first launch or copy.
extern "C" int64_t linetr_debug_stage_workspace_bytes(const LinetrHandle* h, int32_t N, int32_t n_images) {
  if (!h || N < 0 || n_images < 0) return -1;
  return fwd_layout(h, std::max(N, 1), 0, std::max(n_images, 1), nullptr).total;
}

extern "C" int linetr_debug_stage(LinetrHandle* h, int32_t stage, int32_t N, const float* d_in0, const float* d_in1,
                                  const int32_t* h_cu, int32_t n_images, int32_t plan, float* d_out0, float* d_out1, float* d_out2,
                                  int32_t* plan_used, void* d_ws, int64_t ws_bytes, void* stream) {
  if (!h) return fail(LINETR_E_ARG, "debug_stage: null handle");
  if (h->cfg.bn_batch_stats) return fail(LINETR_E_ARG, "debug_stage: a training-mode handle (bn_batch_stats = 1) is not served");
  if (stage != LINETR_STAGE_TAIL && stage != LINETR_STAGE_SIG) return fail(LINETR_E_ARG, "debug_stage: stage must be 0 (tail) or 1 (sig)");
  if (N < 0 || N > INT32_MAX / (HEADS * POOLW)) return fail(LINETR_E_ARG, "debug_stage: row count must be 0 .. %d", INT32_MAX / (HEADS * POOLW));
  const bool sig = stage == LINETR_STAGE_SIG;
  SigAttnPlan p{};
  if (sig) {
    if (int e = check_cu(h_cu, n_images)) return e;
    if (h_cu[n_images] != N) return fail(LINETR_E_ARG, "debug_stage: cu_sub does not end at N");
    const bool eight_waves = plan == (SIGK_FUSED | LINETR_SIG_EIGHT_WAVES);
    if (eight_waves) plan = SIGK_FUSED;
    if (plan < -1 || (plan & ~LINETR_STAGE_FOLD_NEXT) > SIGK_FUSED)
      return fail(LINETR_E_ARG, "debug_stage: plan must be -1 or a kernel 0 .. 4 (+ %d: fold_next; 4 + %d: eight compute waves)",
                  LINETR_STAGE_FOLD_NEXT, LINETR_SIG_EIGHT_WAVES);
    int max_n = 0;
    for (int i = 0; i < n_images; ++i) max_n = std::max(max_n, h_cu[i + 1] - h_cu[i]);
    p = sig_attn_plan(h, n_images, N, max_n);
    if (plan >= 0) {
      const int kernel = plan & ~LINETR_STAGE_FOLD_NEXT;
      // (a fused plan reads no q/k/v rows: its attention kernel stays the dispatcher's, as in every plan sig_attn_plan makes)
      p.fused = kernel == SIGK_FUSED;
      if (!p.fused) p.attn = kernel;
      p.fold_next = (plan & LINETR_STAGE_FOLD_NEXT) != 0;
      p.eight_waves = eight_waves;
      if (int e = sig_plan_servable(h, p, N, max_n)) return e;
    }
    if (plan_used) *plan_used = p.kernel() | (p.fold_next ? LINETR_STAGE_FOLD_NEXT : 0) | (p.eight_waves ? LINETR_SIG_EIGHT_WAVES : 0);
  } else if (plan != -1) {
    return fail(LINETR_E_ARG, "debug_stage: the tail has no plan to force (plan must be -1)");
  }
  if (N == 0) return LINETR_OK;
  if (!d_in0 || (!sig && !d_in1) || (sig && !d_out0) || !d_ws) return fail(LINETR_E_ARG, "debug_stage: null pointer");
  if (((uintptr_t)d_in0 | (uintptr_t)d_in1 | (uintptr_t)d_out0 | (uintptr_t)d_out1 | (uintptr_t)d_out2 | (uintptr_t)d_ws) % 16)
    return fail(LINETR_E_ARG, "debug_stage: tensors and the workspace must be 16-byte aligned");
  const int n_cu = sig ? n_images : 1;
  // (a short workspace is an argument error here, like every other refusal of this entry point)
  const int64_t ws_need = linetr_debug_stage_workspace_bytes(h, N, n_cu);
  if (ws_bytes < ws_need)
    return fail(LINETR_E_ARG, "debug_stage: workspace too small (%lld < %lld bytes)", (long long)ws_bytes, (long long)ws_need);
  LT_HIP(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  FwdWs w = fwd_layout(h, N, 0, n_cu, (char*)d_ws);
  const size_t row_bytes = (size_t)N * D * sizeof(float);
  int e = LINETR_OK;
  auto copy = [&](float* dst, const float* src, size_t bytes) {
    if (!e && dst && hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st) != hipSuccess) e = fail(LINETR_E_HIP, "debug_stage: a device copy failed");
  };
  if (!sig) {
    w.lpos = const_cast<float*>(d_in1);   // read only (the second LayerNorm's add2)
    e = value_projection(h, st, N, d_in0, w.att);
    if (!e) e = sentence(h, st, N, w);
    copy(d_out0, w.att, row_bytes); copy(d_out1, w.o, row_bytes); copy(d_out2, w.zA, row_bytes);
  } else {
    // (sig_network writes every other layer's x_out over its input rows: the caller's stay as they are)
    copy(w.zA, d_in0, row_bytes);
    const int* cu_dev = nullptr;
    if (!e) e = cu_on_device(h_cu, nullptr, n_images, w, st, cu_dev);
    w.tap = h->sig.size() > 1 ? d_out1 : nullptr;
    if (!e) e = sig_network(h, st, TokenStage{}, h_cu, cu_dev, n_images, N, d_out0, w, plan >= 0 ? &p : nullptr);
  }
  (void)hipStreamSynchronize(st);
  return e;
}
