// liblinetr_hip.so, translation unit 4 of 6: training and evaluation (C ABI in include/linetr_hip.h).
//   lt_valstep.h    the validation step
//   lt_lossgrad.h   the criterion's gradient
//   lt_hardnet.h    the HardNet criterion, value and gradient
//   lt_linbwd.h     the backward of the 1x1 layers and the descriptor head
//   lt_attnbwd.h    the neighbour-line attention's forward with statistics and its backward
//   lt_bnbwd.h      BatchNorm on batch statistics with its backward
//   lt_descbwd.h    the descriptive layer's CLS token pooling, LayerNorm and GELU with their backwards
//   lt_dropout.h    the dropout instances of that pooling and LayerNorm
//   lt_posbwd.h     the positional encoders' input layer and the token assembly with their backwards
//   lt_gtassign.h   the ground-truth line assignment in front of them
//   lt_fixedsize.h  the fixed-size samples (pseudo-line padding / truncation) in front of that
//   lt_adam.h       the optimizer step behind them, with the gradient norm that can feed it
#include <algorithm>

#include "lt_handle.h"
#include "lt_valstep.h"
#include "lt_lossgrad.h"
#include "lt_hardnet.h"
#include "lt_linbwd.h"
#include "lt_attnbwd.h"
#include "lt_bnbwd.h"
#include "lt_descbwd.h"
#include "lt_dropout.h"
#include "lt_posbwd.h"
#include "lt_gtassign.h"
#include "lt_fixedsize.h"
#include "lt_adam.h"

using namespace lt;

// =============================================================================================
// validation step (lt_valstep.h)
// =============================================================================================

namespace {
constexpr int VS_MAX_N = 32768;   // n^2 dot products per item are indexed in 64 bits; the grids stay far inside their limits
constexpr int VS_MAX_B = 65535;   // grid.z / grid.y
struct ValOutLayout { int64_t o_scalars, o_count, o_counts, o_scores, total; };
ValOutLayout val_out_layout(int B) {
  ValOutLayout L{};
  Carve c;
  L.o_scalars = c.take(3 * 8);
  L.o_count = c.take(8);
  L.o_counts = c.take((int64_t)B * 4 * 4);
  L.o_scores = c.take((int64_t)B * 3 * 8);
  L.total = c.o;
  return L;
}
// workspace: device image of the result block | dots | norms | per-row results | argmins | match01
struct ValWsLayout { int64_t o_out, o_dots, o_sq0, o_sq1, o_pos, o_neg, o_rarg, o_rmin, o_carg, o_gt, o_m01, total; };
ValWsLayout val_ws_layout(int B, int n) {
  ValWsLayout L{};
  const int64_t rows = align_up((int64_t)B * n * 4, 256);
  Carve c;
  L.o_out = c.take(val_out_layout(B).total);
  L.o_dots = c.take((int64_t)B * n * n * 4);
  L.o_sq0 = c.take(rows);
  L.o_sq1 = c.take(rows);
  L.o_pos = c.take(2 * rows);
  L.o_neg = c.take(2 * rows);
  L.o_rarg = c.take(rows);
  L.o_rmin = c.take(rows);
  L.o_carg = c.take(rows);
  L.o_gt = c.take(rows);
  L.o_m01 = c.take(rows);
  L.total = c.o + 256;
  return L;
}
bool val_dims_ok(int B, int n) { return B > 0 && B <= VS_MAX_B && n > 0 && n <= VS_MAX_N; }

// The prologue of the criterion entry points (linetr_val_step, linetr_desc_loss_grad, linetr_hardnet_loss_grad), for `who`.  First their refusals, every one
// before the first launch (out_need / ws_need: what the entry point's own _output_bytes / _workspace_bytes answer, safe for any shape) ...
int criterion_check(const char* who, int n0, int n1, int B, const float* d_desc0, const float* d_desc1, const float* d_assign,
                    const void* h_pinned_out, int64_t pinned_bytes, int64_t out_need, const void* d_ws, int64_t ws_bytes, int64_t ws_need) {
  if (n0 != n1) return fail(LINETR_E_ARG, "%s: %d and %d sub-lines (the criterion stacks D on D^T: one n for both sides)", who, n0, n1);
  if (!val_dims_ok(B, n0)) return fail(LINETR_E_ARG, "%s: bad shape B=%d n=%d (B 1..%d, n 1..%d)", who, B, n0, VS_MAX_B, VS_MAX_N);
  if (!d_desc0 || !d_desc1 || !d_assign || !h_pinned_out || !d_ws) return fail(LINETR_E_ARG, "%s: null pointer", who);
  if (pinned_bytes < out_need) return fail(LINETR_E_ARG, "%s: output block too small (need %lld)", who, (long long)out_need);
  if (ws_bytes < ws_need) return fail(LINETR_E_ARG, "%s: workspace too small (need %lld)", who, (long long)ws_need);
  return LINETR_OK;
}
// ... then the dot products and squared norms both read
int criterion_dots(LinetrHandle* h, hipStream_t st, const float* d_desc0, const float* d_desc1, int B, int n, float* dots, float* sq0, float* sq1) {
  const int tiles = cdiv(n, 64);
  ProfScope ps(h, st, "val_dot", 2.0 * B * n * n * D, 4.0 * B * (2.0 * n * D + (double)n * n));
  hipLaunchKernelGGL(val_dot_kernel, dim3(tiles, tiles, B), dim3(256), 0, st, d_desc0, d_desc1, n, dots, sq0, sq1);
  LT_LAUNCH_CHECK();
  return LINETR_OK;
}
}  // namespace

extern "C" int64_t linetr_val_step_workspace_bytes(int32_t B, int32_t n) {
  return val_dims_ok(B, n) ? val_ws_layout(B, n).total : 0;
}

extern "C" int64_t linetr_val_step_output_bytes(int32_t B, int64_t* h_offsets) {
  const ValOutLayout L = val_out_layout(std::min(std::max(B, 0), VS_MAX_B));
  if (h_offsets) { h_offsets[0] = L.o_scalars; h_offsets[1] = L.o_count; h_offsets[2] = L.o_counts; h_offsets[3] = L.o_scores; }
  return L.total;
}

extern "C" int linetr_val_step(LinetrHandle* h, const float* d_desc0, int32_t n0, const float* d_desc1, int32_t n1, const float* d_assign,
                               int32_t B, double nn_thresh, int32_t mutual, float* d_row_pos, float* d_row_neg, int32_t* d_match01,
                               void* h_pinned_out, int64_t pinned_bytes, void* d_ws, int64_t ws_bytes, void* stream) {
  if (int e = criterion_check("val_step", n0, n1, B, d_desc0, d_desc1, d_assign, h_pinned_out, pinned_bytes, linetr_val_step_output_bytes(B, nullptr),
                              d_ws, ws_bytes, linetr_val_step_workspace_bytes(B, n0))) return e;
  const int n = n0;
  const ValOutLayout O = val_out_layout(B);
  const ValWsLayout W = val_ws_layout(B, n);
  hipStream_t st = (hipStream_t)stream;
  if (h) LT_HIP(hipSetDevice(h->device));
  char* base = (char*)d_ws;
  float* dots = (float*)(base + W.o_dots);
  float* sq0 = (float*)(base + W.o_sq0);
  float* sq1 = (float*)(base + W.o_sq1);
  float* row_pos = d_row_pos ? d_row_pos : (float*)(base + W.o_pos);
  float* row_neg = d_row_neg ? d_row_neg : (float*)(base + W.o_neg);
  int* row_arg = (int*)(base + W.o_rarg);
  float* row_min = (float*)(base + W.o_rmin);
  int* col_arg = (int*)(base + W.o_carg);
  int* row_gt = (int*)(base + W.o_gt);
  int* match01 = d_match01 ? d_match01 : (int*)(base + W.o_m01);
  char* dout = base + W.o_out;
  const ValOut out{(double*)(dout + O.o_scalars), (long long*)(dout + O.o_count), (int*)(dout + O.o_counts), (double*)(dout + O.o_scores)};
  if (int e = criterion_dots(h, st, d_desc0, d_desc1, B, n, dots, sq0, sq1)) return e;
  {
    ProfScope ps(h, st, "val_select", 0, 16.0 * B * n * n);
    hipLaunchKernelGGL(val_select_kernel, dim3(cdiv(n, VS_ROWS) + cdiv(n, VS_COLS), B), dim3(256), 0, st, (const float*)dots, (const float*)sq0,
                       (const float*)sq1, d_assign, n, row_pos, row_neg, row_arg, row_min, col_arg, row_gt);
    LT_LAUNCH_CHECK();
  }
  {
    ProfScope ps(h, st, "val_final", 0, 44.0 * B * n);
    hipLaunchKernelGGL(val_final_kernel, dim3(B + 1), dim3(256), 0, st, (const float*)row_pos, (const float*)row_neg, (const int*)row_arg,
                       (const float*)row_min, (const int*)col_arg, (const int*)row_gt, d_assign, B, n, nn_thresh, mutual, match01, out);
    LT_LAUNCH_CHECK();
  }
  LT_HIP(hipMemcpyAsync(h_pinned_out, dout, (size_t)O.total, hipMemcpyDeviceToHost, st));
  return LINETR_OK;
}

extern "C" int linetr_assign_from_matches(LinetrHandle* h, const int32_t* d_lmatches, int32_t B, int32_t M, int32_t n, float* d_assign,
                                          void* stream) {
  // (B * M pairs, one thread each: the grid's x extent bounds M)
  if (!val_dims_ok(B, n) || M < 0 || ((int64_t)B * M + 255) / 256 > INT32_MAX)
    return fail(LINETR_E_ARG, "assign_from_matches: bad shape B=%d M=%d n=%d", B, M, n);
  if (!d_assign || (M > 0 && !d_lmatches)) return fail(LINETR_E_ARG, "assign_from_matches: null pointer");
  hipStream_t st = (hipStream_t)stream;
  if (h) LT_HIP(hipSetDevice(h->device));
  LT_HIP(hipMemsetAsync(d_assign, 0, (size_t)B * (n + 1) * (n + 1) * 4, st));
  if (M > 0) {
    hipLaunchKernelGGL(val_assign_kernel, dim3((unsigned)(((int64_t)B * M + 255) / 256)), dim3(256), 0, st, d_lmatches, B, M, n, d_assign);
    LT_LAUNCH_CHECK();
  }
  return LINETR_OK;
}

// =============================================================================================
// gradient of the criterion (lt_lossgrad.h)
// =============================================================================================

namespace {
constexpr int64_t LG_OUT_BYTES = 32;   // f64 [3] loss, hardest_positive, hardest_negative | i64 V
// workspace: device image of the result block | dots | norms (val_dot_kernel writes them) | per-anchor records
struct LossGradWsLayout { int64_t o_out, o_dots, o_sq0, o_sq1, o_pos, o_neg, o_ties, o_arg, total; };
LossGradWsLayout loss_grad_ws_layout(int B, int n) {
  LossGradWsLayout L{};
  const int64_t rows = align_up((int64_t)B * n * 4, 256);
  Carve c;
  L.o_out = c.take(LG_OUT_BYTES);
  L.o_dots = c.take((int64_t)B * n * n * 4);
  L.o_sq0 = c.take(rows);
  L.o_sq1 = c.take(rows);
  L.o_pos = c.take(2 * rows);
  L.o_neg = c.take(2 * rows);
  L.o_ties = c.take(2 * rows);
  L.o_arg = c.take(2 * rows);
  L.total = c.o + 256;
  return L;
}
}  // namespace

extern "C" int64_t linetr_desc_loss_grad_workspace_bytes(int32_t B, int32_t n) {
  return val_dims_ok(B, n) ? loss_grad_ws_layout(B, n).total : 0;
}

extern "C" int linetr_desc_loss_grad(LinetrHandle* h, const float* d_desc0, int32_t n0, const float* d_desc1, int32_t n1, const float* d_assign,
                                     int32_t B, const float* d_upstream, float* d_grad0, float* d_grad1, void* h_pinned_out,
                                     int64_t pinned_bytes, void* d_ws, int64_t ws_bytes, void* stream) {
  if (int e = criterion_check("desc_loss_grad", n0, n1, B, d_desc0, d_desc1, d_assign, h_pinned_out, pinned_bytes, LG_OUT_BYTES, d_ws, ws_bytes,
                              linetr_desc_loss_grad_workspace_bytes(B, n0))) return e;
  const int n = n0;
  const LossGradWsLayout W = loss_grad_ws_layout(B, n);
  hipStream_t st = (hipStream_t)stream;
  if (h) LT_HIP(hipSetDevice(h->device));
  char* base = (char*)d_ws;
  float* dots = (float*)(base + W.o_dots);
  float* row_pos = (float*)(base + W.o_pos);
  float* row_neg = (float*)(base + W.o_neg);
  int* row_ties = (int*)(base + W.o_ties);
  int* row_arg = (int*)(base + W.o_arg);
  double* scalars = (double*)(base + W.o_out);
  long long* count = (long long*)(base + W.o_out + 24);
  if (int e = criterion_dots(h, st, d_desc0, d_desc1, B, n, dots, (float*)(base + W.o_sq0), (float*)(base + W.o_sq1))) return e;
  {
    ProfScope ps(h, st, "lossgrad_select", 0, 16.0 * B * n * n);
    hipLaunchKernelGGL(lg_select_kernel, dim3(cdiv(n, VS_ROWS) + cdiv(n, VS_COLS), B), dim3(256), 0, st, (const float*)dots, d_assign, n,
                       row_pos, row_neg, row_ties, row_arg);
    LT_LAUNCH_CHECK();
  }
  {
    ProfScope ps(h, st, "lossgrad_loss", 0, 16.0 * B * n);
    hipLaunchKernelGGL(lg_loss_kernel, dim3(1), dim3(256), 0, st, (const float*)row_pos, (const float*)row_neg, B, n, scalars, count);
    LT_LAUNCH_CHECK();
  }
  if (d_grad0 || d_grad1) {
    const int sides = (d_grad0 ? 1 : 0) + (d_grad1 ? 1 : 0);
    ProfScope ps(h, st, "lossgrad_grad", 0, sides * 4.0 * B * (2.0 * n * n + (double)n * D));
    hipLaunchKernelGGL(lg_grad_kernel, dim3(cdiv(n, 64), 2, B), dim3(256), 0, st, d_desc0, d_desc1, (const float*)dots, d_assign, n,
                       (const float*)row_pos, (const int*)row_ties, (const int*)row_arg, (const long long*)count, d_upstream, d_grad0, d_grad1);
    LT_LAUNCH_CHECK();
  }
  LT_HIP(hipMemcpyAsync(h_pinned_out, scalars, (size_t)LG_OUT_BYTES, hipMemcpyDeviceToHost, st));
  return LINETR_OK;
}

// =============================================================================================
// the HardNet criterion, value and gradient (lt_hardnet.h)
// =============================================================================================

namespace {
constexpr int64_t HN_OUT_BYTES = 40;   // f64 [3] loss, hardest_positive, hardest_negative | i64 [2] V, live anchors
// workspace: device image of the result block | dots | norms (val_dot_kernel writes them) | per-line records
struct HardnetWsLayout { int64_t o_out, o_dots, o_sq0, o_sq1, o_pos, o_neg, o_arg, o_min, o_cnt, o_live, o_share, total; };
HardnetWsLayout hardnet_ws_layout(int B, int n) {
  HardnetWsLayout L{};
  const int64_t rows = align_up((int64_t)B * n * 4, 256);
  Carve c;
  L.o_out = c.take(HN_OUT_BYTES);
  L.o_dots = c.take((int64_t)B * n * n * 4);
  L.o_sq0 = c.take(rows);
  L.o_sq1 = c.take(rows);
  L.o_pos = c.take(2 * rows);
  L.o_neg = c.take(2 * rows);
  L.o_arg = c.take(2 * rows);
  L.o_min = c.take(2 * rows);
  L.o_cnt = c.take(2 * rows);
  L.o_live = c.take(2 * rows);
  L.o_share = c.take(2 * rows);
  L.total = c.o + 256;
  return L;
}
}  // namespace

extern "C" int64_t linetr_hardnet_loss_grad_workspace_bytes(int32_t B, int32_t n) {
  return val_dims_ok(B, n) ? hardnet_ws_layout(B, n).total : 0;
}

extern "C" int linetr_hardnet_loss_grad(LinetrHandle* h, const float* d_desc0, int32_t n0, const float* d_desc1, int32_t n1,
                                        const float* d_assign, int32_t B, const float* d_upstream, float* d_grad0, float* d_grad1,
                                        float* d_row_pos, float* d_row_neg, int32_t* d_row_arg, void* h_pinned_out, int64_t pinned_bytes,
                                        void* d_ws, int64_t ws_bytes, void* stream) {
  if (int e = criterion_check("hardnet_loss_grad", n0, n1, B, d_desc0, d_desc1, d_assign, h_pinned_out, pinned_bytes, HN_OUT_BYTES, d_ws,
                              ws_bytes, linetr_hardnet_loss_grad_workspace_bytes(B, n0))) return e;
  const int n = n0;
  const HardnetWsLayout W = hardnet_ws_layout(B, n);
  hipStream_t st = (hipStream_t)stream;
  if (h) LT_HIP(hipSetDevice(h->device));
  char* base = (char*)d_ws;
  float* dots = (float*)(base + W.o_dots);
  float* line_pos = d_row_pos ? d_row_pos : (float*)(base + W.o_pos);
  float* row_neg = d_row_neg ? d_row_neg : (float*)(base + W.o_neg);
  int* line_arg = d_row_arg ? d_row_arg : (int*)(base + W.o_arg);
  float* line_min = (float*)(base + W.o_min);
  int* line_cnt = (int*)(base + W.o_cnt);
  int* live_arg = (int*)(base + W.o_live);
  float* neg_share = (float*)(base + W.o_share);
  double* scalars = (double*)(base + W.o_out);
  long long* count = (long long*)(base + W.o_out + 24);
  if (int e = criterion_dots(h, st, d_desc0, d_desc1, B, n, dots, (float*)(base + W.o_sq0), (float*)(base + W.o_sq1))) return e;
  {
    ProfScope ps(h, st, "hardnet_select", 0, 8.0 * B * n * n);
    hipLaunchKernelGGL(hn_select_kernel, dim3(cdiv(n, VS_ROWS) + cdiv(n, VS_COLS), B), dim3(256), 0, st, (const float*)dots, d_assign, n,
                       line_pos, line_arg, line_min, line_cnt);
    LT_LAUNCH_CHECK();
  }
  {
    ProfScope ps(h, st, "hardnet_resolve", 0, 40.0 * B * n);
    hipLaunchKernelGGL(hn_resolve_kernel, dim3(cdiv(2 * n, 256), B), dim3(256), 0, st, (const float*)line_pos, (const int*)line_arg,
                       (const float*)line_min, (const int*)line_cnt, n, row_neg, live_arg, neg_share);
    LT_LAUNCH_CHECK();
  }
  {
    ProfScope ps(h, st, "hardnet_loss", 0, 24.0 * B * n);
    hipLaunchKernelGGL(hn_loss_kernel, dim3(1), dim3(256), 0, st, (const float*)line_pos, (const float*)row_neg, (const int*)line_arg, B, n,
                       scalars, count);
    LT_LAUNCH_CHECK();
  }
  if (d_grad0 || d_grad1) {
    const int sides = (d_grad0 ? 1 : 0) + (d_grad1 ? 1 : 0);
    ProfScope ps(h, st, "hardnet_grad", 0, sides * 4.0 * B * (2.0 * n * n + (double)n * D));
    hipLaunchKernelGGL(hn_grad_kernel, dim3(cdiv(n, 64), 2, B), dim3(256), 0, st, d_desc0, d_desc1, (const float*)dots, d_assign, n,
                       (const int*)live_arg, (const float*)line_min, (const float*)neg_share, (const long long*)count, d_upstream, d_grad0,
                       d_grad1);
    LT_LAUNCH_CHECK();
  }
  LT_HIP(hipMemcpyAsync(h_pinned_out, scalars, (size_t)HN_OUT_BYTES, hipMemcpyDeviceToHost, st));
  return LINETR_OK;
}

// =============================================================================================
// backward of a point-wise linear layer and of the descriptor head (lt_linbwd.h)
// =============================================================================================

namespace {
constexpr int64_t LB_MAX_ROWS = (int64_t)1 << 30;
// workspace: per-chunk tiles of dW | per-chunk column sums
struct LinBwdWsLayout { int chunks; int64_t o_dw, o_db, total; };
LinBwdWsLayout lin_bwd_ws_layout(int64_t rows, int N, int K) {
  LinBwdWsLayout L{};
  L.chunks = (int)((rows + LB_CHUNK - 1) / LB_CHUNK);
  Carve c;
  L.o_dw = c.take((int64_t)L.chunks * N * K * 4);
  L.o_db = c.take((int64_t)L.chunks * N * 4);
  L.total = c.o + 256;
  return L;
}
bool lin_dims_ok(int64_t rows, int N, int K) {
  return rows >= 1 && rows <= LB_MAX_ROWS && N > 0 && K > 0 && N % 64 == 0 && K % 32 == 0 && N <= 1024 && K <= 1024;
}
bool lin_stride_ok(int64_t ld, int width) { return ld >= width && ld % 4 == 0; }

// the argument checks of the layer's backward, for `who`; LINETR_OK: nothing is wrong
int lin_bwd_check(const char* who, const float* d_x, int64_t ldx, const float* d_W, const float* d_g, int64_t ldg, const float* d_mask,
                  int64_t rows, int N, int K, const float* d_dx, const float* d_dW, const float* d_db, const void* d_ws, int64_t ws_bytes) {
  if (!lin_dims_ok(rows, N, K))
    return fail(LINETR_E_ARG, "%s: bad shape rows=%lld N=%d K=%d (rows 1..2^30, N %% 64 == 0, K %% 32 == 0, both <= 1024)", who, (long long)rows, N, K);
  if (!lin_stride_ok(ldx, K) || !lin_stride_ok(ldg, N))
    return fail(LINETR_E_ARG, "%s: row strides %lld / %lld (at least the width, multiples of 4 floats)", who, (long long)ldx, (long long)ldg);
  if (!d_x || !d_W || !d_g) return fail(LINETR_E_ARG, "%s: null pointer", who);
  if ((d_dW || d_db) && !d_ws) return fail(LINETR_E_ARG, "%s: the weight and bias gradients need the workspace", who);
  if (!aligned16(d_x) || !aligned16(d_W) || !aligned16(d_g) || !aligned16(d_mask) || !aligned16(d_dx) || !aligned16(d_dW) ||
      !aligned16(d_db) || !aligned16(d_ws))
    return fail(LINETR_E_ARG, "%s: every tensor must be 16-byte aligned", who);
  if ((d_dW || d_db) && ws_bytes < lin_bwd_ws_layout(rows, N, K).total)
    return fail(LINETR_E_ARG, "%s: workspace too small (need %lld)", who, (long long)lin_bwd_ws_layout(rows, N, K).total);
  return LINETR_OK;
}

// the launches of the layer's backward; the arguments have been checked
int lin_bwd_launch(LinetrHandle* h, hipStream_t st, const float* d_x, int64_t ldx, const float* d_W, const float* d_g, int64_t ldg,
                   const float* d_mask, int64_t rows, int N, int K, float* d_dx, float* d_dW, float* d_db, void* d_ws) {
  if (d_dx) {
    ProfScope ps(h, st, "linbwd_dx", 2.0 * rows * N * K, 4.0 * (rows * (double)(N + K) + (double)N * K));
    hipLaunchKernelGGL(lb_dx_kernel, dim3((unsigned)((rows + 63) / 64), cdiv(K, 64)), dim3(256), 0, st, d_g, d_mask, ldg, d_W, rows, N, K,
                       d_dx, ldx);
    LT_LAUNCH_CHECK();
  }
  if (d_dW || d_db) {
    const LinBwdWsLayout L = lin_bwd_ws_layout(rows, N, K);
    float* dw_part = d_dW ? (float*)((char*)d_ws + L.o_dw) : nullptr;
    float* db_part = d_db ? (float*)((char*)d_ws + L.o_db) : nullptr;
    {
      ProfScope ps(h, st, "linbwd_dw_partial", d_dW ? 2.0 * rows * N * K : 0.0, 4.0 * (rows * (double)(N + K) + (double)L.chunks * N * K));
      hipLaunchKernelGGL(lb_dw_partial_kernel, dim3(L.chunks, N / 64, d_dW ? cdiv(K, 64) : 1), dim3(256), 0, st, d_g, d_mask, ldg, d_x, ldx,
                         rows, N, K, dw_part, db_part);
      LT_LAUNCH_CHECK();
    }
    {
      const int64_t quads = (d_dW ? (int64_t)N * K / 4 : 0) + (d_db ? N / 4 : 0);
      ProfScope ps(h, st, "linbwd_dw_reduce", 0, 4.0 * (L.chunks + 1) * (double)N * K);
      hipLaunchKernelGGL(lb_dw_reduce_kernel, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, st, (const float*)dw_part,
                         (const float*)db_part, L.chunks, N, K, d_dW, d_db);
      LT_LAUNCH_CHECK();
    }
  }
  return LINETR_OK;
}
}  // namespace

extern "C" int32_t linetr_linear_backward_chunk_rows(void) { return LB_CHUNK; }

extern "C" int64_t linetr_linear_backward_workspace_bytes(int64_t rows, int32_t N, int32_t K) {
  return lin_dims_ok(rows, N, K) ? lin_bwd_ws_layout(rows, N, K).total : 0;
}

extern "C" int linetr_linear_forward(LinetrHandle* h, const float* d_x, int64_t ldx, const float* d_W, const float* d_b, int64_t rows,
                                     int32_t N, int32_t K, int32_t act, float* d_y, int64_t ldy, void* stream) {
  // every refusal comes before the first launch
  if (!lin_dims_ok(rows, N, K))
    return fail(LINETR_E_ARG, "linear_forward: bad shape rows=%lld N=%d K=%d (rows 1..2^30, N %% 64 == 0, K %% 32 == 0, both <= 1024)", (long long)rows, N, K);
  if (act != 0 && act != 1) return fail(LINETR_E_ARG, "linear_forward: act %d (0 none, 1 ReLU)", act);
  if (!lin_stride_ok(ldx, K) || !lin_stride_ok(ldy, N))
    return fail(LINETR_E_ARG, "linear_forward: row strides %lld / %lld (at least the width, multiples of 4 floats)", (long long)ldx, (long long)ldy);
  if (!d_x || !d_W || !d_y) return fail(LINETR_E_ARG, "linear_forward: null pointer");
  if (!aligned16(d_x) || !aligned16(d_W) || !aligned16(d_b) || !aligned16(d_y)) return fail(LINETR_E_ARG, "linear_forward: every tensor must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  if (h) LT_HIP(hipSetDevice(h->device));
  ProfScope ps(h, st, "linear_fwd", 2.0 * rows * N * K, 4.0 * (rows * (double)(N + K) + (double)N * K));
  hipLaunchKernelGGL(lb_fwd_kernel<false>, dim3((unsigned)((rows + 63) / 64), N / 64), dim3(256), 0, st, d_x, ldx, d_W, d_b, rows, N, K, act, d_y,
                     ldy, (const float*)nullptr, (float*)nullptr);
  LT_LAUNCH_CHECK();
  return LINETR_OK;
}

extern "C" int linetr_linear_backward(LinetrHandle* h, const float* d_x, int64_t ldx, const float* d_W, const float* d_g, int64_t ldg,
                                      const float* d_mask, int64_t rows, int32_t N, int32_t K, float* d_dx, float* d_dW, float* d_db,
                                      void* d_ws, int64_t ws_bytes, void* stream) {
  const int rc = lin_bwd_check("linear_backward", d_x, ldx, d_W, d_g, ldg, d_mask, rows, N, K, d_dx, d_dW, d_db, d_ws, ws_bytes);
  if (rc != LINETR_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (h) LT_HIP(hipSetDevice(h->device));
  return lin_bwd_launch(h, st, d_x, ldx, d_W, d_g, ldg, d_mask, rows, N, K, d_dx, d_dW, d_db, d_ws);
}

namespace {
int64_t head_gy_bytes(int64_t rows) { return align_up(rows * D * 4, 256); }
int head_launch(LinetrHandle* h, hipStream_t st, const float* d_x, const float* d_W, const float* d_b, int64_t rows, float* d_desc,
                const float* d_g, float* d_gy) {
  ProfScope ps(h, st, d_g ? "head_fwd_bwd_norm" : "head_fwd", 2.0 * rows * D * D, 4.0 * ((d_g ? 4.0 : 2.0) * rows * D + (double)D * D));
  hipLaunchKernelGGL(lb_fwd_kernel<true>, dim3((unsigned)((rows + LB_HEAD_ROWS - 1) / LB_HEAD_ROWS)), dim3(256), 0, st, d_x, (int64_t)D, d_W, d_b,
                     rows, D, D, 0, d_desc, (int64_t)D, d_g, d_gy);
  LT_LAUNCH_CHECK();
  return LINETR_OK;
}
}  // namespace

extern "C" int64_t linetr_head_backward_workspace_bytes(int64_t rows) {
  return lin_dims_ok(rows, D, D) ? head_gy_bytes(rows) + lin_bwd_ws_layout(rows, D, D).total : 0;
}

extern "C" int linetr_head_forward(LinetrHandle* h, const float* d_x, const float* d_W, const float* d_b, int64_t rows, float* d_desc,
                                   void* stream) {
  if (!lin_dims_ok(rows, D, D)) return fail(LINETR_E_ARG, "head_forward: bad rows=%lld (1..2^30)", (long long)rows);
  if (!d_x || !d_W || !d_b || !d_desc) return fail(LINETR_E_ARG, "head_forward: null pointer");
  if (!aligned16(d_x) || !aligned16(d_W) || !aligned16(d_b) || !aligned16(d_desc)) return fail(LINETR_E_ARG, "head_forward: every tensor must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  if (h) LT_HIP(hipSetDevice(h->device));
  return head_launch(h, st, d_x, d_W, d_b, rows, d_desc, nullptr, nullptr);
}

extern "C" int linetr_head_backward(LinetrHandle* h, const float* d_x, const float* d_W, const float* d_b, const float* d_g, int64_t rows,
                                    float* d_dx, float* d_dW, float* d_db, void* d_ws, int64_t ws_bytes, void* stream) {
  if (!lin_dims_ok(rows, D, D)) return fail(LINETR_E_ARG, "head_backward: bad rows=%lld (1..2^30)", (long long)rows);
  if (!d_x || !d_W || !d_b || !d_g || !d_ws) return fail(LINETR_E_ARG, "head_backward: null pointer");
  if (!aligned16(d_b)) return fail(LINETR_E_ARG, "head_backward: every tensor must be 16-byte aligned");
  if (ws_bytes < linetr_head_backward_workspace_bytes(rows))
    return fail(LINETR_E_ARG, "head_backward: workspace too small (need %lld)", (long long)linetr_head_backward_workspace_bytes(rows));
  float* gy = (float*)d_ws;
  char* rest = (char*)d_ws + head_gy_bytes(rows);
  const int rc = lin_bwd_check("head_backward", d_x, D, d_W, d_g, D, nullptr, rows, D, D, d_dx, d_dW, d_db, rest, ws_bytes - head_gy_bytes(rows));
  if (rc != LINETR_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (h) LT_HIP(hipSetDevice(h->device));
  const int rl = head_launch(h, st, d_x, d_W, d_b, rows, nullptr, d_g, gy);
  if (rl != LINETR_OK) return rl;
  return lin_bwd_launch(h, st, d_x, D, d_W, gy, D, nullptr, rows, D, D, d_dx, d_dW, d_db, rest);
}

// =============================================================================================
// neighbour-line attention for training: forward with statistics, backward (lt_attnbwd.h)
// =============================================================================================

namespace {
constexpr int64_t AB_MAX_ROWS = 0x7fffffff;      // cu_sub is int32
constexpr int AB_MAX_IMAGES = 4096;              // every block walks cu_sub (ab_find_tile): the walk, and the grid of N / 128 + n_images, stay small
int64_t attn_delta_bytes(int64_t N) { return align_up(N * HEADS * 4, 256); }
bool attn_stride_ok(int64_t ld) { return ld >= D && ld % 4 == 0; }
// tiles of 128 rows of any split of N rows into n_images images, at most
unsigned attn_tiles(int64_t N, int n_images) { return (unsigned)(N / ATT_QT + n_images); }
}  // namespace

extern "C" int64_t linetr_sig_attention_backward_workspace_bytes(int64_t N) {
  return N >= 0 && N <= AB_MAX_ROWS ? attn_delta_bytes(N) + 256 : 0;
}

extern "C" int linetr_sig_attention_forward(LinetrHandle* h, const float* d_q, int64_t ldq, const float* d_k, int64_t ldk, const float* d_v,
                                            int64_t ldv, const int32_t* d_cu_sub, int32_t n_images, int64_t N, float* d_msg, int64_t ldo,
                                            float* d_lse, void* stream) {
  // every refusal comes before the first launch
  if (n_images < 1 || n_images > AB_MAX_IMAGES || N < 0 || N > AB_MAX_ROWS)
    return fail(LINETR_E_ARG, "sig_attention_forward: n_images=%d N=%lld (1 <= n_images <= %d, 0 <= N < 2^31)", n_images, (long long)N, AB_MAX_IMAGES);
  if (!d_q || !d_k || !d_v || !d_cu_sub || !d_msg || !d_lse) return fail(LINETR_E_ARG, "sig_attention_forward: null pointer");
  if (!attn_stride_ok(ldq) || !attn_stride_ok(ldk) || !attn_stride_ok(ldv) || !attn_stride_ok(ldo))
    return fail(LINETR_E_ARG, "sig_attention_forward: row strides %lld / %lld / %lld / %lld (at least 256, multiples of 4 floats)", (long long)ldq,
                (long long)ldk, (long long)ldv, (long long)ldo);
  if (!aligned16(d_q) || !aligned16(d_k) || !aligned16(d_v) || !aligned16(d_msg) || !aligned16(d_lse))
    return fail(LINETR_E_ARG, "sig_attention_forward: every tensor must be 16-byte aligned");
  if (N == 0) return LINETR_OK;
  hipStream_t st = (hipStream_t)stream;
  if (h) LT_HIP(hipSetDevice(h->device));
  ProfScope ps(h, st, "sig_attn_fwd_lse", 0, 4.0 * N * (4.0 * D + HEADS));
  hipLaunchKernelGGL(ab_fwd_kernel, dim3(attn_tiles(N, n_images), HEADS), dim3(256), 0, st, d_q, ldq, d_k, ldk, d_v, ldv, (const int*)d_cu_sub,
                     n_images, d_msg, ldo, d_lse);
  LT_LAUNCH_CHECK();
  return LINETR_OK;
}

extern "C" int linetr_sig_attention_backward(LinetrHandle* h, const float* d_q, int64_t ldq, const float* d_k, int64_t ldk, const float* d_v,
                                             int64_t ldv, const float* d_msg, int64_t ldo, const float* d_lse, const float* d_g, int64_t ldg,
                                             const int32_t* d_cu_sub, int32_t n_images, int64_t N, float* d_dq, int64_t lddq, float* d_dk,
                                             int64_t lddk, float* d_dv, int64_t lddv, void* d_ws, int64_t ws_bytes, void* stream) {
  if (n_images < 1 || n_images > AB_MAX_IMAGES || N < 0 || N > AB_MAX_ROWS)
    return fail(LINETR_E_ARG, "sig_attention_backward: n_images=%d N=%lld (1 <= n_images <= %d, 0 <= N < 2^31)", n_images, (long long)N, AB_MAX_IMAGES);
  if (!d_q || !d_k || !d_v || !d_msg || !d_lse || !d_g || !d_cu_sub || !d_ws) return fail(LINETR_E_ARG, "sig_attention_backward: null pointer");
  if (!attn_stride_ok(ldq) || !attn_stride_ok(ldk) || !attn_stride_ok(ldv) || !attn_stride_ok(ldo) || !attn_stride_ok(ldg) ||
      (d_dq && !attn_stride_ok(lddq)) || (d_dk && !attn_stride_ok(lddk)) || (d_dv && !attn_stride_ok(lddv)))
    return fail(LINETR_E_ARG, "sig_attention_backward: every row stride must be at least 256 and a multiple of 4 floats");
  if (!aligned16(d_q) || !aligned16(d_k) || !aligned16(d_v) || !aligned16(d_msg) || !aligned16(d_lse) || !aligned16(d_g) || !aligned16(d_dq) ||
      !aligned16(d_dk) || !aligned16(d_dv) || !aligned16(d_ws))
    return fail(LINETR_E_ARG, "sig_attention_backward: every tensor must be 16-byte aligned");
  if (ws_bytes < linetr_sig_attention_backward_workspace_bytes(N))
    return fail(LINETR_E_ARG, "sig_attention_backward: workspace too small (need %lld)", (long long)linetr_sig_attention_backward_workspace_bytes(N));
  if (N == 0 || (!d_dq && !d_dk && !d_dv)) return LINETR_OK;
  hipStream_t st = (hipStream_t)stream;
  if (h) LT_HIP(hipSetDevice(h->device));
  float* delta = (float*)d_ws;
  const dim3 grid(attn_tiles(N, n_images), HEADS);
  if (d_dq || d_dk) {       // dV reads P alone
    ProfScope ps(h, st, "sig_attn_bwd_delta", 0, 4.0 * N * (2.0 * D + HEADS));
    hipLaunchKernelGGL(ab_delta_kernel, dim3((unsigned)((N + 31) / 32), HEADS), dim3(64), 0, st, d_g, ldg, d_msg, ldo, N, delta);
    LT_LAUNCH_CHECK();
  }
  if (d_dk || d_dv) {
    ProfScope ps(h, st, "sig_attn_bwd_dkv", 0, 4.0 * N * (6.0 * D + 2.0 * HEADS));
    hipLaunchKernelGGL(ab_dkv_kernel, grid, dim3(256), 0, st, d_q, ldq, d_k, ldk, d_v, ldv, d_g, ldg, d_lse, (const float*)delta,
                       (const int*)d_cu_sub, n_images, d_dk, lddk, d_dv, lddv);
    LT_LAUNCH_CHECK();
  }
  if (d_dq) {
    ProfScope ps(h, st, "sig_attn_bwd_dq", 0, 4.0 * N * (5.0 * D + 2.0 * HEADS));
    hipLaunchKernelGGL(ab_dq_kernel, grid, dim3(256), 0, st, d_q, ldq, d_k, ldk, d_v, ldv, d_g, ldg, d_lse, (const float*)delta,
                       (const int*)d_cu_sub, n_images, d_dq, lddq);
    LT_LAUNCH_CHECK();
  }
  return LINETR_OK;
}

// =============================================================================================
// BatchNorm1d (+ ReLU) for training: forward that keeps z and the statistics (lt_bntrain.h), backward (lt_bnbwd.h)
// =============================================================================================

namespace {
constexpr int64_t BN_MAX_ROWS = (int64_t)1 << 30;
// workspace: per-chunk partial sums [chunks][2 C] float64 | per-channel coefficients (forward: alpha | beta'; backward: k1 | k2 | k3)
struct BnWsLayout { int chunks; int64_t o_partial, o_coef, total; };
BnWsLayout bn_ws_layout(int64_t rows, int C) {
  BnWsLayout L{};
  L.chunks = bn_row_chunks(rows);
  Carve c;
  L.o_partial = c.take((int64_t)L.chunks * 2 * C * 8);
  L.o_coef = c.take((int64_t)3 * C * 4);
  L.total = c.o + 256;
  return L;
}
bool bn_dims_ok(int64_t rows, int C) { return rows <= BN_MAX_ROWS && bn_channels_ok(C); }
}  // namespace

extern "C" int64_t linetr_bn_forward_workspace_bytes(int64_t rows, int32_t C) { return bn_dims_ok(rows, C) ? bn_ws_layout(rows, C).total : 0; }
extern "C" int64_t linetr_bn_backward_workspace_bytes(int64_t rows, int32_t C) { return bn_dims_ok(rows, C) ? bn_ws_layout(rows, C).total : 0; }

extern "C" int linetr_bn_forward(LinetrHandle* h, const float* d_z, int64_t ldz, int64_t rows, int32_t C, const float* d_gamma,
                                 const float* d_beta, float eps, float momentum, float* d_running, int32_t mode, int32_t relu, float* d_y,
                                 int64_t ldy, double* d_save, void* d_ws, int64_t ws_bytes, void* stream) {
  // every refusal comes before the first launch
  if (!bn_dims_ok(rows, C))
    return fail(LINETR_E_ARG, "bn_forward: bad shape rows=%lld C=%d (rows <= 2^30, 4 <= C <= %d, C %% 4 == 0)", (long long)rows, C, BN_MAX_CHANNELS);
  if (mode != LINETR_BN_TRAIN && mode != LINETR_BN_EVAL) return fail(LINETR_E_ARG, "bn_forward: mode %d (0 batch statistics, 1 running statistics)", mode);
  if (relu != 0 && relu != 1) return fail(LINETR_E_ARG, "bn_forward: relu %d (0 none, 1 ReLU)", relu);
  if (!(eps > 0.f) || !(momentum >= 0.f && momentum <= 1.f)) return fail(LINETR_E_ARG, "bn_forward: eps %g (> 0), momentum %g (0 .. 1)", eps, momentum);
  if (!bn_rows_ok(d_z, ldz, C) || !bn_rows_ok(d_y, ldy, C))
    return fail(LINETR_E_ARG, "bn_forward: row strides %lld / %lld (at least C = %d, multiples of 4 floats) on 16-byte aligned bases", (long long)ldz,
                (long long)ldy, C);
  if (!d_z || !d_gamma || !d_beta || !d_y || !d_save || !d_ws) return fail(LINETR_E_ARG, "bn_forward: null pointer");
  if (mode == LINETR_BN_EVAL && !d_running) return fail(LINETR_E_ARG, "bn_forward: eval mode reads the running statistics");
  if (!aligned16(d_gamma) || !aligned16(d_beta) || !aligned16(d_running) || !aligned16(d_save) || !aligned16(d_ws))
    return fail(LINETR_E_ARG, "bn_forward: every tensor must be 16-byte aligned");
  if (ws_bytes < linetr_bn_forward_workspace_bytes(rows, C))
    return fail(LINETR_E_ARG, "bn_forward: workspace too small (need %lld)", (long long)linetr_bn_forward_workspace_bytes(rows, C));
  if (rows <= 0) return LINETR_OK;
  const BnWsLayout L = bn_ws_layout(rows, C);
  hipStream_t st = (hipStream_t)stream;
  if (h) LT_HIP(hipSetDevice(h->device));
  return bn_forward_launch(st, h, (double*)((char*)d_ws + L.o_partial), (float*)((char*)d_ws + L.o_coef), d_z, ldz, rows, C, d_gamma, d_beta, eps,
                           momentum, d_running, mode == LINETR_BN_EVAL, nullptr, d_save, relu != 0, d_y, ldy);
}

extern "C" int linetr_bn_backward(LinetrHandle* h, const float* d_z, int64_t ldz, const float* d_y, int64_t ldy, const float* d_g, int64_t ldg,
                                  const double* d_save, const float* d_gamma, int64_t rows, int32_t C, int32_t mode, float* d_dz,
                                  int64_t lddz, float* d_dgamma, float* d_dbeta, void* d_ws, int64_t ws_bytes, void* stream) {
  if (!bn_dims_ok(rows, C))
    return fail(LINETR_E_ARG, "bn_backward: bad shape rows=%lld C=%d (rows <= 2^30, 4 <= C <= %d, C %% 4 == 0)", (long long)rows, C, BN_MAX_CHANNELS);
  if (mode != LINETR_BN_TRAIN && mode != LINETR_BN_EVAL) return fail(LINETR_E_ARG, "bn_backward: mode %d (0 batch statistics, 1 running statistics)", mode);
  if (!bn_rows_ok(d_z, ldz, C) || !bn_rows_ok(d_g, ldg, C) || (d_y && !bn_rows_ok(d_y, ldy, C)) || (d_dz && !bn_rows_ok(d_dz, lddz, C)))
    return fail(LINETR_E_ARG, "bn_backward: every row stride must be at least C = %d and a multiple of 4 floats, every base 16-byte aligned", C);
  if (!d_z || !d_g || !d_save || !d_gamma || !d_ws) return fail(LINETR_E_ARG, "bn_backward: null pointer");
  if (!aligned16(d_save) || !aligned16(d_gamma) || !aligned16(d_dgamma) || !aligned16(d_dbeta) || !aligned16(d_ws))
    return fail(LINETR_E_ARG, "bn_backward: every tensor must be 16-byte aligned");
  if (ws_bytes < linetr_bn_backward_workspace_bytes(rows, C))
    return fail(LINETR_E_ARG, "bn_backward: workspace too small (need %lld)", (long long)linetr_bn_backward_workspace_bytes(rows, C));
  if (rows <= 0 || (!d_dz && !d_dgamma && !d_dbeta)) return LINETR_OK;
  const BnWsLayout L = bn_ws_layout(rows, C);
  hipStream_t st = (hipStream_t)stream;
  if (h) LT_HIP(hipSetDevice(h->device));
  double* partial = (double*)((char*)d_ws + L.o_partial);
  float* coef = (float*)((char*)d_ws + L.o_coef);
  const bool eval = mode == LINETR_BN_EVAL;
  const bool sums = !eval || d_dgamma || d_dbeta;      // eval mode: dz needs no sum
  const double tensors = d_y ? 3.0 : 2.0;
  if (sums) {
    ProfScope ps(h, st, "bn_bwd_partial", 0, 4.0 * tensors * rows * C);
    hipLaunchKernelGGL(bn_bwd_partial_kernel, dim3(L.chunks, cdiv(C / 4, BNB_QUADS)), dim3(256), 0, st, d_g, ldg, d_y, ldy, d_z, ldz, d_save, rows,
                       (int)C, partial);
    LT_LAUNCH_CHECK();
  }
  {
    ProfScope ps(h, st, "bn_bwd_finalize", 0, 16.0 * L.chunks * C);
    hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3((C + 255) / 256), dim3(256), 0, st, (const double*)partial, sums ? L.chunks : 0, (int)C, rows,
                       d_gamma, d_save, (int)eval, d_dgamma, d_dbeta, coef);
    LT_LAUNCH_CHECK();
  }
  if (d_dz) {
    ProfScope ps(h, st, "bn_bwd_apply", 0, 4.0 * (tensors + (eval ? 0.0 : 1.0)) * rows * C);
    hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3((unsigned)((rows * (C / 4) + 255) / 256)), dim3(256), 0, st, d_g, ldg, d_y, ldy, d_z, ldz, d_save,
                       (const float*)coef, rows, (int)C, (int)eval, d_dz, lddz);
    LT_LAUNCH_CHECK();
  }
  return LINETR_OK;
}

// =============================================================================================
// the line descriptive layer for training: CLS token pooling, LayerNorm, GELU, each forward and backward (lt_descbwd.h)
// =============================================================================================

namespace {
constexpr int64_t CP_MAX_L = (int64_t)1 << 24;      // L S <= 2^32 rows are indexed in 64 bits; the grid of L / 4 blocks stays small
constexpr int64_t LN_MAX_ROWS = (int64_t)1 << 30;
constexpr int64_t DROP_MAX_ROWS = ((int64_t)1 << 31) - 1;     // a row is one 32-bit word of the Philox counter
bool cp_dims_ok(int64_t L, int S) { return L >= 0 && L <= CP_MAX_L && S >= 1 && S <= CP_MAX_S; }
int64_t ln_chunks(int64_t rows) { return (rows + LN_CHUNK - 1) / LN_CHUNK; }

// The refusals of the pooling and LayerNorm entry points, with and without dropout, for `who`: every one before the first launch.
int cp_fwd_check(const char* who, const float* d_x, int64_t ldx, const float* d_u, int64_t ldu, int64_t L, int S, const float* d_pooled,
                 const float* d_lse) {
  if (!cp_dims_ok(L, S)) return fail(LINETR_E_ARG, "%s: bad shape L=%lld S=%d (0 <= L <= 2^24, 1 <= S <= %d)", who, (long long)L, S, CP_MAX_S);
  if (!lin_stride_ok(ldx, D) || !lin_stride_ok(ldu, HEADS * D))
    return fail(LINETR_E_ARG, "%s: row strides %lld / %lld (at least 256 / 1024, multiples of 4 floats)", who, (long long)ldx, (long long)ldu);
  if (!d_x || !d_u || !d_pooled || !d_lse) return fail(LINETR_E_ARG, "%s: null pointer", who);
  if (!aligned16(d_x) || !aligned16(d_u) || !aligned16(d_pooled) || !aligned16(d_lse))
    return fail(LINETR_E_ARG, "%s: every tensor must be 16-byte aligned", who);
  return LINETR_OK;
}
int cp_bwd_check(const char* who, const float* d_x, int64_t ldx, const float* d_u, int64_t ldu, const float* d_pooled, const float* d_lse,
                 const float* d_dpooled, int64_t L, int S, const float* d_dx, int64_t lddx, const float* d_du, int64_t lddu) {
  if (!cp_dims_ok(L, S)) return fail(LINETR_E_ARG, "%s: bad shape L=%lld S=%d (0 <= L <= 2^24, 1 <= S <= %d)", who, (long long)L, S, CP_MAX_S);
  if (!lin_stride_ok(ldx, D) || !lin_stride_ok(ldu, HEADS * D) || (d_dx && !lin_stride_ok(lddx, D)) || (d_du && !lin_stride_ok(lddu, HEADS * D)))
    return fail(LINETR_E_ARG, "%s: every row stride must be at least the width (256 tokens, 1024 u) and a multiple of 4 floats", who);
  if (!d_x || !d_u || !d_pooled || !d_lse || !d_dpooled) return fail(LINETR_E_ARG, "%s: null pointer", who);
  if (!aligned16(d_x) || !aligned16(d_u) || !aligned16(d_pooled) || !aligned16(d_lse) || !aligned16(d_dpooled) || !aligned16(d_dx) || !aligned16(d_du))
    return fail(LINETR_E_ARG, "%s: every tensor must be 16-byte aligned", who);
  return LINETR_OK;
}
int ln_fwd_check(const char* who, const float* d_a, int64_t lda, const float* d_r, int64_t ldr, const float* d_gamma, const float* d_beta, float eps,
                 int64_t rows, int C, const float* d_y, int64_t ldy, const float* d_stats) {
  if (C != D || rows < 0 || rows > LN_MAX_ROWS) return fail(LINETR_E_ARG, "%s: bad shape rows=%lld C=%d (0 <= rows <= 2^30, C = 256)", who, (long long)rows, C);
  if (!(eps > 0.f)) return fail(LINETR_E_ARG, "%s: eps %g (> 0)", who, eps);
  if (!lin_stride_ok(lda, D) || (d_r && !lin_stride_ok(ldr, D)) || !lin_stride_ok(ldy, D))
    return fail(LINETR_E_ARG, "%s: every row stride must be at least 256 and a multiple of 4 floats", who);
  if (!d_a || !d_gamma || !d_beta || !d_y || !d_stats) return fail(LINETR_E_ARG, "%s: null pointer", who);
  if (!aligned16(d_a) || !aligned16(d_r) || !aligned16(d_gamma) || !aligned16(d_beta) || !aligned16(d_y) || !aligned16(d_stats))
    return fail(LINETR_E_ARG, "%s: every tensor must be 16-byte aligned", who);
  return LINETR_OK;
}
// (d_dx / d_dx2: the one data gradient of the plain backward, the two of the dropout one)
int ln_bwd_check(const char* who, const float* d_a, int64_t lda, const float* d_r, int64_t ldr, const float* d_stats, const float* d_gamma,
                 const float* d_g, int64_t ldg, int64_t rows, int C, const float* d_dx, int64_t lddx, const float* d_dx2, int64_t lddx2,
                 const float* d_dgamma, const float* d_dbeta, const void* d_ws, int64_t ws_bytes) {
  if (C != D || rows < 0 || rows > LN_MAX_ROWS) return fail(LINETR_E_ARG, "%s: bad shape rows=%lld C=%d (0 <= rows <= 2^30, C = 256)", who, (long long)rows, C);
  if (!lin_stride_ok(lda, D) || (d_r && !lin_stride_ok(ldr, D)) || !lin_stride_ok(ldg, D) || (d_dx && !lin_stride_ok(lddx, D)) ||
      (d_dx2 && !lin_stride_ok(lddx2, D)))
    return fail(LINETR_E_ARG, "%s: every row stride must be at least 256 and a multiple of 4 floats", who);
  if (!d_a || !d_stats || !d_gamma || !d_g) return fail(LINETR_E_ARG, "%s: null pointer", who);
  const bool sums = d_dgamma || d_dbeta;
  if (sums && !d_ws) return fail(LINETR_E_ARG, "%s: the gamma and beta gradients need the workspace", who);
  if (!aligned16(d_a) || !aligned16(d_r) || !aligned16(d_stats) || !aligned16(d_gamma) || !aligned16(d_g) || !aligned16(d_dx) || !aligned16(d_dx2) ||
      !aligned16(d_dgamma) || !aligned16(d_dbeta) || !aligned16(d_ws))
    return fail(LINETR_E_ARG, "%s: every tensor must be 16-byte aligned", who);
  if (sums && ws_bytes < linetr_layer_norm_backward_workspace_bytes(rows, C))
    return fail(LINETR_E_ARG, "%s: workspace too small (need %lld)", who, (long long)linetr_layer_norm_backward_workspace_bytes(rows, C));
  return LINETR_OK;
}
// the second launch of both LayerNorm backwards: the chunks' partial rows added in ascending order (no rows: zeros)
int ln_reduce(LinetrHandle* h, hipStream_t st, const float* partial, int chunks, float* d_dgamma, float* d_dbeta) {
  ProfScope ps(h, st, "layer_norm_bwd_reduce", 0, 4.0 * (chunks + 1) * 2.0 * D);
  hipLaunchKernelGGL(ln_reduce_kernel, dim3(2), dim3(256), 0, st, partial, chunks, d_dgamma, d_dbeta);
  LT_LAUNCH_CHECK();
  return LINETR_OK;
}
// LinetrDropout as the kernels take it, or a refusal
int drop_args(const char* who, const LinetrDropout* drop, int site, DropArgs* out) {
  if (!drop) return fail(LINETR_E_ARG, "%s: null dropout state", who);
  if (site < 0 || site > 2) return fail(LINETR_E_ARG, "%s: site %d (0: attention weights, 1 / 2: in front of the first / second LayerNorm)", who, site);
  if (!std::isfinite(drop->scale) || drop->scale < 1.f) return fail(LINETR_E_ARG, "%s: scale %g (1 / (1 - p) with 0 <= p < 1)", who, drop->scale);
  *out = DropArgs{(uint32_t)(drop->seed & 0xffffffffu), (uint32_t)(drop->seed >> 32), drop->call, drop->threshold, drop->scale};
  return LINETR_OK;
}
}  // namespace

extern "C" int64_t linetr_layer_norm_backward_workspace_bytes(int64_t rows, int32_t C) {
  return C == D && rows >= 0 && rows <= LN_MAX_ROWS ? align_up(ln_chunks(rows) * 2 * D * 4, 256) + 256 : 0;
}

namespace {
// The pooling and the LayerNorm, forward and backward: one call each behind its plain entry point (`dropout` false: drop, site, d_kept,
// d_dkept and the second data gradient are not looked at) and its dropout one (lt_dropout.h).
int cp_fwd_call(const char* who, LinetrHandle* h, const float* d_x, int64_t ldx, const float* d_u, int64_t ldu, int64_t L, int S, bool dropout,
                const LinetrDropout* drop, float* d_pooled, float* d_kept, float* d_lse, void* stream) {
  if (int e = cp_fwd_check(who, d_x, ldx, d_u, ldu, L, S, d_pooled, d_lse)) return e;
  DropArgs dr{};
  if (dropout) {
    if (!d_kept || !aligned16(d_kept)) return fail(LINETR_E_ARG, "%s: kept must be a 16-byte aligned [L][4] tensor", who);
    if (int e = drop_args(who, drop, 0, &dr)) return e;
  }
  if (L == 0) return LINETR_OK;
  hipStream_t st = (hipStream_t)stream;
  if (h) LT_HIP(hipSetDevice(h->device));
  ProfScope ps(h, st, dropout ? "cls_pool_dropout_fwd" : "cls_pool_train_fwd", 2.0 * HEADS * 2.0 * L * S * D,
               4.0 * L * ((double)S * D + 2.0 * HEADS * D + (dropout ? 2 : 1) * HEADS));
  const dim3 grid((unsigned)((L + CP_SEGS - 1) / CP_SEGS));
  if (dropout) hipLaunchKernelGGL(cp_drop_fwd_kernel, grid, dim3(256), 0, st, d_x, ldx, d_u, ldu, L, S, dr, d_pooled, d_kept, d_lse);
  else hipLaunchKernelGGL(cp_fwd_kernel, grid, dim3(256), 0, st, d_x, ldx, d_u, ldu, L, S, d_pooled, d_lse);
  LT_LAUNCH_CHECK();
  return LINETR_OK;
}

int cp_bwd_call(const char* who, LinetrHandle* h, const float* d_x, int64_t ldx, const float* d_u, int64_t ldu, const float* d_pooled,
                const float* d_lse, const float* d_kept, const float* d_dpooled, const float* d_dkept, int64_t L, int S, bool dropout,
                const LinetrDropout* drop, float* d_dx, int64_t lddx, float* d_du, int64_t lddu, void* stream) {
  if (int e = cp_bwd_check(who, d_x, ldx, d_u, ldu, d_pooled, d_lse, d_dpooled, L, S, d_dx, lddx, d_du, lddu)) return e;
  DropArgs dr{};
  if (dropout) {
    if (!d_kept || !aligned16(d_kept) || !aligned16(d_dkept))
      return fail(LINETR_E_ARG, "%s: kept and dkept must be 16-byte aligned [L][4] tensors (dkept may be null)", who);
    if (int e = drop_args(who, drop, 0, &dr)) return e;
  }
  if (L == 0 || (!d_dx && !d_du)) return LINETR_OK;
  hipStream_t st = (hipStream_t)stream;
  if (h) LT_HIP(hipSetDevice(h->device));
  ProfScope ps(h, st, dropout ? "cls_pool_dropout_bwd" : "cls_pool_train_bwd", 2.0 * HEADS * 4.0 * L * S * D,
               4.0 * L * ((d_dx ? 2.0 : 1.0) * S * D + 4.0 * HEADS * D + (dropout ? 3 : 1) * HEADS));
  const dim3 grid((unsigned)((L + CP_SEGS - 1) / CP_SEGS));
  if (dropout)
    hipLaunchKernelGGL(cp_drop_bwd_kernel, grid, dim3(256), 0, st, d_x, ldx, d_u, ldu, d_pooled, d_lse, d_kept, d_dpooled, d_dkept, L, S, dr, d_dx,
                       lddx, d_du, lddu);
  else hipLaunchKernelGGL(cp_bwd_kernel, grid, dim3(256), 0, st, d_x, ldx, d_u, ldu, d_pooled, d_lse, d_dpooled, L, S, d_dx, lddx, d_du, lddu);
  LT_LAUNCH_CHECK();
  return LINETR_OK;
}

int ln_fwd_call(const char* who, LinetrHandle* h, const float* d_a, int64_t lda, const float* d_r, int64_t ldr, const float* d_gamma,
                const float* d_beta, float eps, int64_t rows, int C, bool dropout, const LinetrDropout* drop, int site, float* d_y, int64_t ldy,
                float* d_stats, void* stream) {
  if (int e = ln_fwd_check(who, d_a, lda, d_r, ldr, d_gamma, d_beta, eps, rows, C, d_y, ldy, d_stats)) return e;
  DropArgs dr{};
  if (dropout)
    if (int e = drop_args(who, drop, site, &dr)) return e;
  if (rows == 0) return LINETR_OK;
  hipStream_t st = (hipStream_t)stream;
  if (h) LT_HIP(hipSetDevice(h->device));
  ProfScope ps(h, st, dropout ? "layer_norm_dropout_fwd" : "layer_norm_fwd", 0, 4.0 * rows * ((d_r ? 3.0 : 2.0) * D + 2));
  const dim3 grid((unsigned)((rows + LN_ROWS - 1) / LN_ROWS));
  if (dropout)
    hipLaunchKernelGGL(ln_drop_fwd_kernel, grid, dim3(256), 0, st, d_a, lda, d_r, ldr, d_gamma, d_beta, eps, rows, dr, (uint32_t)site, d_y, ldy,
                       d_stats);
  else hipLaunchKernelGGL(ln_fwd_kernel, grid, dim3(256), 0, st, d_a, lda, d_r, ldr, d_gamma, d_beta, eps, rows, d_y, ldy, d_stats);
  LT_LAUNCH_CHECK();
  return LINETR_OK;
}

// (d_dr: the gradient of v = a + residual, the plain backward's one data gradient; d_da: that of a under dropout, r dv)
int ln_bwd_call(const char* who, LinetrHandle* h, const float* d_a, int64_t lda, const float* d_r, int64_t ldr, const float* d_stats,
                const float* d_gamma, const float* d_g, int64_t ldg, int64_t rows, int C, bool dropout, const LinetrDropout* drop, int site,
                float* d_da, int64_t ldda, float* d_dr, int64_t lddr, float* d_dgamma, float* d_dbeta, void* d_ws, int64_t ws_bytes, void* stream) {
  if (int e = ln_bwd_check(who, d_a, lda, d_r, ldr, d_stats, d_gamma, d_g, ldg, rows, C, d_da, ldda, d_dr, lddr, d_dgamma, d_dbeta, d_ws, ws_bytes))
    return e;
  DropArgs dr{};
  if (dropout)
    if (int e = drop_args(who, drop, site, &dr)) return e;
  const bool sums = d_dgamma || d_dbeta;
  if (!d_da && !d_dr && !sums) return LINETR_OK;
  hipStream_t st = (hipStream_t)stream;
  if (h) LT_HIP(hipSetDevice(h->device));
  const int chunks = (int)ln_chunks(rows);
  float* partial = sums ? (float*)d_ws : nullptr;
  if (rows > 0) {
    ProfScope ps(h, st, dropout ? "layer_norm_dropout_bwd" : "layer_norm_bwd", 0,
                 4.0 * rows * ((d_r ? 3.0 : 2.0) * D + 2 + (d_da ? D : 0) + (d_dr ? D : 0)));
    if (dropout)
      hipLaunchKernelGGL(ln_drop_bwd_kernel, dim3((unsigned)chunks), dim3(256), 0, st, d_a, lda, d_r, ldr, d_stats, d_gamma, d_g, ldg, rows, dr,
                         (uint32_t)site, d_da, ldda, d_dr, lddr, partial);
    else
      hipLaunchKernelGGL(ln_bwd_kernel, dim3((unsigned)chunks), dim3(256), 0, st, d_a, lda, d_r, ldr, d_stats, d_gamma, d_g, ldg, rows, d_dr, lddr,
                         partial);
    LT_LAUNCH_CHECK();
  }
  return sums ? ln_reduce(h, st, partial, chunks, d_dgamma, d_dbeta) : LINETR_OK;
}
}  // namespace

extern "C" int linetr_cls_pool_train_forward(LinetrHandle* h, const float* d_x, int64_t ldx, const float* d_u, int64_t ldu, int64_t L, int32_t S,
                                             float* d_pooled, float* d_lse, void* stream) {
  return cp_fwd_call("cls_pool_train_forward", h, d_x, ldx, d_u, ldu, L, S, false, nullptr, d_pooled, nullptr, d_lse, stream);
}

extern "C" int linetr_cls_pool_train_backward(LinetrHandle* h, const float* d_x, int64_t ldx, const float* d_u, int64_t ldu, const float* d_pooled,
                                              const float* d_lse, const float* d_dpooled, int64_t L, int32_t S, float* d_dx, int64_t lddx,
                                              float* d_du, int64_t lddu, void* stream) {
  return cp_bwd_call("cls_pool_train_backward", h, d_x, ldx, d_u, ldu, d_pooled, d_lse, nullptr, d_dpooled, nullptr, L, S, false, nullptr, d_dx,
                     lddx, d_du, lddu, stream);
}

extern "C" int linetr_layer_norm_forward(LinetrHandle* h, const float* d_a, int64_t lda, const float* d_r, int64_t ldr, const float* d_gamma,
                                         const float* d_beta, float eps, int64_t rows, int32_t C, float* d_y, int64_t ldy, float* d_stats,
                                         void* stream) {
  return ln_fwd_call("layer_norm_forward", h, d_a, lda, d_r, ldr, d_gamma, d_beta, eps, rows, C, false, nullptr, 0, d_y, ldy, d_stats, stream);
}

extern "C" int linetr_layer_norm_backward(LinetrHandle* h, const float* d_a, int64_t lda, const float* d_r, int64_t ldr, const float* d_stats,
                                          const float* d_gamma, const float* d_g, int64_t ldg, int64_t rows, int32_t C, float* d_dx,
                                          int64_t lddx, float* d_dgamma, float* d_dbeta, void* d_ws, int64_t ws_bytes, void* stream) {
  return ln_bwd_call("layer_norm_backward", h, d_a, lda, d_r, ldr, d_stats, d_gamma, d_g, ldg, rows, C, false, nullptr, 0, nullptr, 0, d_dx, lddx,
                     d_dgamma, d_dbeta, d_ws, ws_bytes, stream);
}

extern "C" int linetr_cls_pool_dropout_forward(LinetrHandle* h, const float* d_x, int64_t ldx, const float* d_u, int64_t ldu, int64_t L, int32_t S,
                                               const LinetrDropout* drop, float* d_pooled, float* d_kept, float* d_lse, void* stream) {
  return cp_fwd_call("cls_pool_dropout_forward", h, d_x, ldx, d_u, ldu, L, S, true, drop, d_pooled, d_kept, d_lse, stream);
}

extern "C" int linetr_cls_pool_dropout_backward(LinetrHandle* h, const float* d_x, int64_t ldx, const float* d_u, int64_t ldu, const float* d_pooled,
                                                const float* d_lse, const float* d_kept, const float* d_dpooled, const float* d_dkept, int64_t L,
                                                int32_t S, const LinetrDropout* drop, float* d_dx, int64_t lddx, float* d_du, int64_t lddu,
                                                void* stream) {
  return cp_bwd_call("cls_pool_dropout_backward", h, d_x, ldx, d_u, ldu, d_pooled, d_lse, d_kept, d_dpooled, d_dkept, L, S, true, drop, d_dx, lddx,
                     d_du, lddu, stream);
}

extern "C" int linetr_layer_norm_dropout_forward(LinetrHandle* h, const float* d_a, int64_t lda, const float* d_r, int64_t ldr, const float* d_gamma,
                                                 const float* d_beta, float eps, int64_t rows, int32_t C, const LinetrDropout* drop, int32_t site,
                                                 float* d_y, int64_t ldy, float* d_stats, void* stream) {
  return ln_fwd_call("layer_norm_dropout_forward", h, d_a, lda, d_r, ldr, d_gamma, d_beta, eps, rows, C, true, drop, site, d_y, ldy, d_stats, stream);
}

extern "C" int linetr_layer_norm_dropout_backward(LinetrHandle* h, const float* d_a, int64_t lda, const float* d_r, int64_t ldr, const float* d_stats,
                                                  const float* d_gamma, const float* d_g, int64_t ldg, int64_t rows, int32_t C,
                                                  const LinetrDropout* drop, int32_t site, float* d_da, int64_t ldda, float* d_dr, int64_t lddr,
                                                  float* d_dgamma, float* d_dbeta, void* d_ws, int64_t ws_bytes, void* stream) {
  return ln_bwd_call("layer_norm_dropout_backward", h, d_a, lda, d_r, ldr, d_stats, d_gamma, d_g, ldg, rows, C, true, drop, site, d_da, ldda, d_dr,
                     lddr, d_dgamma, d_dbeta, d_ws, ws_bytes, stream);
}

extern "C" int linetr_dropout_factors(LinetrHandle* h, const LinetrDropout* drop, int32_t site, int64_t rows, int64_t inner, float* d_out, void* stream) {
  const char* who = "dropout_factors";
  if (rows < 0 || rows > DROP_MAX_ROWS || inner < 1 || inner > DROP_MAX_ROWS || rows * inner > ((int64_t)1 << 38))
    return fail(LINETR_E_ARG, "%s: bad shape rows=%lld inner=%lld (0 <= rows < 2^31, 1 <= inner < 2^31, rows inner <= 2^38)", who, (long long)rows,
                (long long)inner);
  DropArgs dr;
  if (int e = drop_args(who, drop, site, &dr)) return e;
  if (!d_out || !aligned16(d_out)) return fail(LINETR_E_ARG, "%s: the output must be a 16-byte aligned tensor", who);
  if (rows == 0) return LINETR_OK;
  hipStream_t st = (hipStream_t)stream;
  if (h) LT_HIP(hipSetDevice(h->device));
  ProfScope ps(h, st, "dropout_factors", 0, 16.0 * rows * inner);
  hipLaunchKernelGGL(drop_factors_kernel, dim3((unsigned)((rows * inner + 255) / 256)), dim3(256), 0, st, dr, (uint32_t)site, rows, inner, d_out);
  LT_LAUNCH_CHECK();
  return LINETR_OK;
}

namespace {
// forward (d_g null) and backward of GELU share one check and one kernel
int gelu_call(const char* who, LinetrHandle* h, const float* d_z, int64_t ldz, const float* d_g, int64_t ldg, bool backward, int64_t rows, int C,
              float* d_out, int64_t ldo, void* stream) {
  if (rows < 0 || rows > LN_MAX_ROWS || C < 4 || C > 4096 || C % 4 || (rows * (C / 4) + 255) / 256 > INT32_MAX)
    return fail(LINETR_E_ARG, "%s: bad shape rows=%lld C=%d (0 <= rows <= 2^30, 4 <= C <= 4096, C %% 4 == 0)", who, (long long)rows, C);
  if (!lin_stride_ok(ldz, C) || (backward && !lin_stride_ok(ldg, C)) || !lin_stride_ok(ldo, C))
    return fail(LINETR_E_ARG, "%s: every row stride must be at least C = %d and a multiple of 4 floats", who, C);
  if (!d_z || !d_out || (backward && !d_g)) return fail(LINETR_E_ARG, "%s: null pointer", who);
  if (!aligned16(d_z) || !aligned16(d_g) || !aligned16(d_out)) return fail(LINETR_E_ARG, "%s: every tensor must be 16-byte aligned", who);
  if (rows == 0) return LINETR_OK;
  hipStream_t st = (hipStream_t)stream;
  if (h) LT_HIP(hipSetDevice(h->device));
  ProfScope ps(h, st, backward ? "gelu_bwd" : "gelu_fwd", 0, 4.0 * rows * C * (backward ? 3.0 : 2.0));
  hipLaunchKernelGGL(gelu_kernel, dim3((unsigned)((rows * (C / 4) + 255) / 256)), dim3(256), 0, st, d_z, ldz, backward ? d_g : nullptr, ldg, rows, C, d_out,
                     ldo);
  LT_LAUNCH_CHECK();
  return LINETR_OK;
}
}  // namespace

extern "C" int linetr_gelu_forward(LinetrHandle* h, const float* d_z, int64_t ldz, int64_t rows, int32_t C, float* d_y, int64_t ldy, void* stream) {
  return gelu_call("gelu_forward", h, d_z, ldz, nullptr, 0, false, rows, C, d_y, ldy, stream);
}

extern "C" int linetr_gelu_backward(LinetrHandle* h, const float* d_z, int64_t ldz, const float* d_g, int64_t ldg, int64_t rows, int32_t C,
                                    float* d_dz, int64_t lddz, void* stream) {
  return gelu_call("gelu_backward", h, d_z, ldz, d_g, ldg, true, rows, C, d_dz, lddz, stream);
}

// =============================================================================================
// the positional encoders' input layer and the token assembly, each forward and backward (lt_posbwd.h)
// =============================================================================================

namespace {
constexpr int64_t IL_MAX_ROWS = (int64_t)1 << 30;
constexpr int64_t TA_MAX_L = (int64_t)1 << 24;      // L (S + 1) <= 2^32 rows are indexed in 64 bits; the grid of L (S + 1) / 4 blocks stays below 2^31
bool il_dims_ok(int64_t rows, int N, int Kin) {
  return rows >= 0 && rows <= IL_MAX_ROWS && Kin >= 1 && Kin <= IL_MAX_K && N >= 4 && N <= IL_MAX_N && N % 4 == 0;
}
int64_t il_chunks(int64_t rows) { return (rows + IL_CHUNK - 1) / IL_CHUNK; }
bool aligned4(const void* p) { return ((uintptr_t)p & 3) == 0; }
bool ta_dims_ok(int64_t L, int S) { return L >= 0 && L <= TA_MAX_L && S >= 1 && S <= TA_MAX_S; }
int64_t ta_blocks(int64_t L) { return (L + TA_SEGS - 1) / TA_SEGS; }
}  // namespace

extern "C" int32_t linetr_input_layer_chunk_rows(void) { return IL_CHUNK; }

extern "C" int64_t linetr_input_layer_backward_workspace_bytes(int64_t rows, int32_t N, int32_t Kin) {
  return il_dims_ok(rows, N, Kin) ? align_up(il_chunks(rows) * (Kin + 1) * N * 4, 256) + 256 : 0;
}

extern "C" int linetr_input_layer_forward(LinetrHandle* h, const float* d_x, int64_t ldx, const float* d_W, const float* d_b, int64_t rows,
                                          int32_t N, int32_t Kin, float* d_z, int64_t ldz, void* stream) {
  // every refusal comes before the first launch
  if (!il_dims_ok(rows, N, Kin))
    return fail(LINETR_E_ARG, "input_layer_forward: bad shape rows=%lld N=%d Kin=%d (0 <= rows <= 2^30, 1 <= Kin <= 8, N %% 4 == 0, 4 <= N <= 64)",
                (long long)rows, N, Kin);
  if (ldx < Kin || !lin_stride_ok(ldz, N))
    return fail(LINETR_E_ARG, "input_layer_forward: row strides %lld / %lld (x: at least Kin = %d floats; z: at least N = %d, a multiple of 4 floats)",
                (long long)ldx, (long long)ldz, Kin, N);
  if (!d_x || !d_W || !d_z) return fail(LINETR_E_ARG, "input_layer_forward: null pointer");
  if (!aligned4(d_x) || !aligned4(d_W) || !aligned4(d_b) || !aligned16(d_z))
    return fail(LINETR_E_ARG, "input_layer_forward: z must be 16-byte aligned (x, W and b: 4-byte aligned)");
  if (rows == 0) return LINETR_OK;
  hipStream_t st = (hipStream_t)stream;
  if (h) LT_HIP(hipSetDevice(h->device));
  ProfScope ps(h, st, "input_layer_fwd", 2.0 * rows * N * Kin, 4.0 * rows * ((double)N + Kin));
  hipLaunchKernelGGL(il_fwd_kernel, dim3((unsigned)((rows * (N / 4) + 255) / 256)), dim3(256), 0, st, d_x, ldx, d_W, d_b, rows, (int)N, (int)Kin, d_z,
                     ldz);
  LT_LAUNCH_CHECK();
  return LINETR_OK;
}

extern "C" int linetr_input_layer_backward(LinetrHandle* h, const float* d_x, int64_t ldx, const float* d_g, int64_t ldg, int64_t rows, int32_t N,
                                           int32_t Kin, float* d_dW, float* d_db, void* d_ws, int64_t ws_bytes, void* stream) {
  if (!il_dims_ok(rows, N, Kin))
    return fail(LINETR_E_ARG, "input_layer_backward: bad shape rows=%lld N=%d Kin=%d (0 <= rows <= 2^30, 1 <= Kin <= 8, N %% 4 == 0, 4 <= N <= 64)",
                (long long)rows, N, Kin);
  if (ldx < Kin || !lin_stride_ok(ldg, N))
    return fail(LINETR_E_ARG, "input_layer_backward: row strides %lld / %lld (x: at least Kin = %d floats; g: at least N = %d, a multiple of 4 floats)",
                (long long)ldx, (long long)ldg, Kin, N);
  if (!d_x || !d_g) return fail(LINETR_E_ARG, "input_layer_backward: null pointer");
  if ((d_dW || d_db) && !d_ws) return fail(LINETR_E_ARG, "input_layer_backward: the weight and bias gradients need the workspace");
  if (!aligned4(d_x) || !aligned16(d_g) || !aligned4(d_dW) || !aligned4(d_db) || !aligned16(d_ws))
    return fail(LINETR_E_ARG, "input_layer_backward: g and the workspace must be 16-byte aligned (x, dW and db: 4-byte aligned)");
  if ((d_dW || d_db) && ws_bytes < linetr_input_layer_backward_workspace_bytes(rows, N, Kin))
    return fail(LINETR_E_ARG, "input_layer_backward: workspace too small (need %lld)", (long long)linetr_input_layer_backward_workspace_bytes(rows, N, Kin));
  if (!d_dW && !d_db) return LINETR_OK;
  hipStream_t st = (hipStream_t)stream;
  if (h) LT_HIP(hipSetDevice(h->device));
  const int chunks = (int)il_chunks(rows);
  float* partial = (float*)d_ws;
  if (rows > 0) {
    ProfScope ps(h, st, "input_layer_bwd_partial", 2.0 * rows * N * Kin, 4.0 * (rows * ((double)N + Kin) + (double)chunks * (Kin + 1) * N));
    hipLaunchKernelGGL(il_bwd_partial_kernel, dim3((unsigned)chunks), dim3(256), 0, st, d_x, ldx, d_g, ldg, rows, (int)N, (int)Kin, partial);
    LT_LAUNCH_CHECK();
  }
  {      // (no rows: zeros)
    ProfScope ps(h, st, "input_layer_bwd_reduce", 0, 4.0 * (chunks + 1) * (double)(Kin + 1) * N);
    hipLaunchKernelGGL(il_bwd_reduce_kernel, dim3(cdiv((Kin + 1) * N, 64)), dim3(1024), 0, st, (const float*)partial, chunks, (int)N, (int)Kin, d_dW,
                       d_db);
    LT_LAUNCH_CHECK();
  }
  return LINETR_OK;
}

extern "C" int64_t linetr_token_assemble_backward_workspace_bytes(int64_t L) {
  return L >= 0 && L <= TA_MAX_L ? align_up(ta_blocks(L) * D * 4, 256) + 256 : 0;
}

extern "C" int linetr_token_assemble_forward(LinetrHandle* h, const float* d_desc, const float* d_pos, const float* d_cls, int64_t L, int32_t S,
                                             float* d_x, void* stream) {
  // every refusal comes before the first launch
  if (!ta_dims_ok(L, S))
    return fail(LINETR_E_ARG, "token_assemble_forward: bad shape L=%lld S=%d (0 <= L <= 2^24, 1 <= S <= %d)", (long long)L, S, TA_MAX_S);
  if (!d_desc || !d_pos || !d_cls || !d_x) return fail(LINETR_E_ARG, "token_assemble_forward: null pointer");
  if (!aligned16(d_desc) || !aligned16(d_pos) || !aligned16(d_cls) || !aligned16(d_x))
    return fail(LINETR_E_ARG, "token_assemble_forward: every tensor must be 16-byte aligned");
  if (L == 0) return LINETR_OK;
  hipStream_t st = (hipStream_t)stream;
  if (h) LT_HIP(hipSetDevice(h->device));
  ProfScope ps(h, st, "token_assemble_fwd", 0, 4.0 * L * D * (3.0 * S + 1));
  hipLaunchKernelGGL(ta_fwd_kernel, dim3((unsigned)((L * (S + 1) + 3) / 4)), dim3(256), 0, st, d_desc, d_pos, d_cls, L, (int)S, d_x);
  LT_LAUNCH_CHECK();
  return LINETR_OK;
}

extern "C" int linetr_token_assemble_backward(LinetrHandle* h, const float* d_dx, int64_t L, int32_t S, float* d_dtok, float* d_dcls, void* d_ws,
                                              int64_t ws_bytes, void* stream) {
  if (!ta_dims_ok(L, S))
    return fail(LINETR_E_ARG, "token_assemble_backward: bad shape L=%lld S=%d (0 <= L <= 2^24, 1 <= S <= %d)", (long long)L, S, TA_MAX_S);
  if (!d_dx) return fail(LINETR_E_ARG, "token_assemble_backward: null pointer");
  if (d_dcls && !d_ws) return fail(LINETR_E_ARG, "token_assemble_backward: the cls gradient needs the workspace");
  if (!aligned16(d_dx) || !aligned16(d_dtok) || !aligned16(d_dcls) || !aligned16(d_ws))
    return fail(LINETR_E_ARG, "token_assemble_backward: every tensor must be 16-byte aligned");
  if (d_dcls && ws_bytes < linetr_token_assemble_backward_workspace_bytes(L))
    return fail(LINETR_E_ARG, "token_assemble_backward: workspace too small (need %lld)", (long long)linetr_token_assemble_backward_workspace_bytes(L));
  if (!d_dtok && !d_dcls) return LINETR_OK;
  hipStream_t st = (hipStream_t)stream;
  if (h) LT_HIP(hipSetDevice(h->device));
  const int blocks = (int)ta_blocks(L);
  float* partial = d_dcls ? (float*)d_ws : nullptr;
  if (L > 0) {
    ProfScope ps(h, st, "token_assemble_bwd", 0, 4.0 * L * D * ((d_dtok ? 2.0 * S : 0.0) + (d_dcls ? 1.0 : 0.0)));
    hipLaunchKernelGGL(ta_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, st, d_dx, L, (int)S, d_dtok, partial);
    LT_LAUNCH_CHECK();
  }
  if (d_dcls) {      // (no segments: zeros)
    ProfScope ps(h, st, "token_assemble_bwd_reduce", 0, 4.0 * (blocks + 1) * (double)D);
    hipLaunchKernelGGL(ta_reduce_kernel, dim3(D / 64), dim3(1024), 0, st, (const float*)partial, blocks, d_dcls);
    LT_LAUNCH_CHECK();
  }
  return LINETR_OK;
}

// =============================================================================================
// ground-truth line assignment of a homography pair (lt_gtassign.h)
// =============================================================================================

namespace {
// workspace (sized for the double instance): projected lines of both sides | the four angle arrays | ballot words | found
struct GtLayout { int W64; int64_t o_proj0, o_proj1, o_ang, o_words, o_found, total; };
GtLayout gt_layout(int B, int n0, int n1) {
  GtLayout L{};
  L.W64 = cdiv(n1, 64);
  Carve c;
  L.o_proj0 = c.take((int64_t)B * n0 * 4 * 8);
  L.o_proj1 = c.take((int64_t)B * n1 * 4 * 8);
  L.o_ang = c.take((int64_t)B * 2 * ((int64_t)n0 + n1) * 8);
  L.o_words = c.take((int64_t)B * n0 * L.W64 * 8);
  L.o_found = c.take((int64_t)B * 4);
  L.total = c.o + 256;
  return L;
}
bool gt_dims_ok(int B, int n0, int n1) { return B > 0 && B <= VS_MAX_B && n0 > 0 && n0 <= VS_MAX_N && n1 > 0 && n1 <= VS_MAX_N; }

template <typename T>
int gt_assign_launch(LinetrHandle* h, hipStream_t st, const GtLayout& L, const void* d_lines0, int n0, const void* d_lines1, int n1,
                     const double* d_H, int B, const int32_t* d_count0, const int32_t* d_count1, double thres_reprojected,
                     double thres_angdiff, double min_overlap_ratio, int pad, float* d_assign, int32_t* d_lmatches, int M,
                     int32_t* d_found, uint8_t* d_match_dir, void* d_overlap_dir, void* d_proj0, void* d_proj1, char* base) {
  const T* lines0 = (const T*)d_lines0;
  const T* lines1 = (const T*)d_lines1;
  T* proj0 = d_proj0 ? (T*)d_proj0 : (T*)(base + L.o_proj0);
  T* proj1 = d_proj1 ? (T*)d_proj1 : (T*)(base + L.o_proj1);
  T* ang0 = (T*)(base + L.o_ang);
  T* angp0 = ang0 + (int64_t)B * n0;
  T* ang1 = angp0 + (int64_t)B * n0;
  T* angp1 = ang1 + (int64_t)B * n1;
  const bool list = d_lmatches || d_found;
  unsigned long long* words = list ? (unsigned long long*)(base + L.o_words) : nullptr;
  const double pairs = (double)B * n0 * n1;
  {
    ProfScope ps(h, st, "gt_lines", 0, (double)B * ((double)n0 + n1) * (4 * 2 + 2) * sizeof(T));
    hipLaunchKernelGGL(gt_lines_kernel<T>, dim3(cdiv(n0, 256), B), dim3(256), 0, st, lines0, n0, d_H, 0, proj0, ang0, angp0);
    hipLaunchKernelGGL(gt_lines_kernel<T>, dim3(cdiv(n1, 256), B), dim3(256), 0, st, lines1, n1, d_H, 1, proj1, ang1, angp1);
    LT_LAUNCH_CHECK();
  }
  {
    ProfScope ps(h, st, "gt_pair", 0, (d_assign ? 4.0 * B * (n0 + pad) * (n1 + pad) : 0.0) + (d_match_dir ? 2.0 * pairs : 0.0) +
                                          (d_overlap_dir ? 2.0 * pairs * sizeof(T) : 0.0) + (words ? (double)B * n0 * L.W64 * 8 : 0.0));
    hipLaunchKernelGGL(gt_pair_kernel<T>, dim3(cdiv(n1 + pad, 64), cdiv(n0 + pad, GT_ROWS), B), dim3(256), 0, st, lines0, lines1,
                       (const T*)proj0, (const T*)proj1, (const T*)ang0, (const T*)ang1, (const T*)angp0, (const T*)angp1, n0, n1,
                       d_count0, d_count1, (T)thres_reprojected, (T)thres_angdiff, min_overlap_ratio, pad, d_assign, d_match_dir,
                       (T*)d_overlap_dir, words);
    LT_LAUNCH_CHECK();
  }
  if (list) {
    ProfScope ps(h, st, "gt_list", 0, (double)B * n0 * L.W64 * 8 + (d_lmatches ? 8.0 * B * M : 0.0));
    hipLaunchKernelGGL(gt_list_kernel, dim3(B), dim3(256), 0, st, (const unsigned long long*)words, n0, L.W64, M, d_lmatches,
                       d_found ? d_found : (int32_t*)(base + L.o_found));
    LT_LAUNCH_CHECK();
  }
  return LINETR_OK;
}
}  // namespace

extern "C" int64_t linetr_gt_assign_workspace_bytes(int32_t B, int32_t n0, int32_t n1) {
  return gt_dims_ok(B, n0, n1) ? gt_layout(B, n0, n1).total : 0;
}

extern "C" int linetr_gt_assign(LinetrHandle* h, int32_t coord_type, const void* d_lines0, int32_t n0, const void* d_lines1, int32_t n1,
                                const double* d_H, int32_t B, const int32_t* d_count0, const int32_t* d_count1,
                                double thres_reprojected, double thres_angdiff, double min_overlap_ratio, int32_t pad, float* d_assign,
                                int32_t* d_lmatches, int32_t M, int32_t* d_found, uint8_t* d_match_dir, void* d_overlap_dir,
                                void* d_proj0, void* d_proj1, void* d_ws, int64_t ws_bytes, void* stream) {
  // every refusal comes before the first launch
  if (!gt_dims_ok(B, n0, n1))
    return fail(LINETR_E_ARG, "gt_assign: bad shape B=%d n0=%d n1=%d (B 1..%d, n 1..%d)", B, n0, n1, VS_MAX_B, VS_MAX_N);
  if (M < 0) return fail(LINETR_E_ARG, "gt_assign: M = %d", M);
  if (pad != 0 && pad != 1) return fail(LINETR_E_ARG, "gt_assign: pad %d (0, or 1 for the dustbin row and column)", pad);
  if (coord_type != LINETR_COORD_F32 && coord_type != LINETR_COORD_F64)
    return fail(LINETR_E_ARG, "gt_assign: coordinate type %d (0 float32, 1 float64)", coord_type);
  if (!d_lines0 || !d_lines1 || !d_H || !d_ws) return fail(LINETR_E_ARG, "gt_assign: null pointer");
  const GtLayout L = gt_layout(B, n0, n1);
  if (ws_bytes < L.total) return fail(LINETR_E_ARG, "gt_assign: workspace too small (need %lld)", (long long)L.total);
  hipStream_t st = (hipStream_t)stream;
  if (h) LT_HIP(hipSetDevice(h->device));
  if (coord_type == LINETR_COORD_F32)
    return gt_assign_launch<float>(h, st, L, d_lines0, n0, d_lines1, n1, d_H, B, d_count0, d_count1, thres_reprojected, thres_angdiff,
                                   min_overlap_ratio, pad, d_assign, d_lmatches, M, d_found, d_match_dir, d_overlap_dir, d_proj0,
                                   d_proj1, (char*)d_ws);
  return gt_assign_launch<double>(h, st, L, d_lines0, n0, d_lines1, n1, d_H, B, d_count0, d_count1, thres_reprojected, thres_angdiff,
                                  min_overlap_ratio, pad, d_assign, d_lmatches, M, d_found, d_match_dir, d_overlap_dir, d_proj0,
                                  d_proj1, (char*)d_ws);
}

// =============================================================================================
// fixed-size training samples: pseudo-line padding / truncation of the tokeniser's tensors (lt_fixedsize.h)
// =============================================================================================

namespace {
constexpr int FS_MAX_B = 65535, FS_MAX_M = 32768;
struct FsLayout { int64_t o_table, o_nhwc, total; };
FsLayout fs_layout(int B, int height, int width, int dense_is_nhwc) {
  FsLayout L{};
  Carve c;
  L.o_table = c.take((int64_t)B * sizeof(FsImage));
  L.o_nhwc = c.take(dense_is_nhwc ? 0 : (int64_t)B * (height / 8) * (width / 8) * D * 4);
  L.total = c.o;
  return L;
}
bool fs_dims_ok(int B, int height, int width) {
  return B > 0 && B <= FS_MAX_B && height >= 8 && width >= 8 && height % 8 == 0 && width % 8 == 0 && height <= 32768 && width <= 32768;
}
}  // namespace

extern "C" int64_t linetr_fixed_size_workspace_bytes(int32_t n_images, int32_t height, int32_t width, int32_t dense_is_nhwc) {
  if (dense_is_nhwc > 0 && (dense_is_nhwc & ~0xff)) return 0;   // float32 maps only (below): what the call refuses needs no workspace
  return fs_dims_ok(n_images, height, width) ? fs_layout(n_images, height, width, dense_is_nhwc).total : 0;
}

extern "C" int linetr_fixed_size(LinetrHandle* h, const LinetrLineRec* d_recs, const int32_t* h_cu_k, const int32_t* h_cu_n,
                                 const LinetrLineRec* d_pseudo, const LinetrLineRec* h_pseudo, const int32_t* h_cu_p, int32_t B,
                                 int32_t M, int32_t T, double td, const float* d_dense_desc, const float* d_dense_score, int32_t height,
                                 int32_t width, int32_t clip_height, int32_t clip_width, int32_t pseudo_clip_height,
                                 int32_t pseudo_clip_width, int32_t align_corners, int32_t dense_is_nhwc, LinetrTokens out,
                                 int32_t* d_num_klns, int32_t* d_num_slns, void* d_ws, int64_t ws_bytes, void* stream) {
  // every refusal comes before the first launch
  if (dense_is_nhwc > 0 && (dense_is_nhwc & ~0xff))   // the training samples are float32: a half map read as float32 would be silent garbage
    return fail(LINETR_E_ARG, "fixed_size: dense_is_nhwc = 0x%x: the maps must be float32 (no LINETR_DENSE_F16 / LINETR_DENSE_BF16 here)", (unsigned)dense_is_nhwc);
  if (!fs_dims_ok(B, height, width)) return fail(LINETR_E_ARG, "fixed_size: bad shape B=%d height=%d width=%d", B, height, width);
  if (M < 1 || M > FS_MAX_M || T < 1 || T > 4096 || !(td > 0)) return fail(LINETR_E_ARG, "fixed_size: bad max_sublines / max_tokens / token_distance");
  if (((int64_t)B * M * T + 3) / 4 > INT32_MAX) return fail(LINETR_E_ARG, "fixed_size: B * max_sublines * max_tokens beyond 2^33 tokens");
  if (!h_cu_k || !h_cu_n || !h_cu_p || !d_dense_desc || !d_dense_score || !out.klines || !out.length || !out.angles || !out.sublines ||
      !out.pnt || !out.mask || !out.resp || !out.angle_sub || !out.desc || !out.score || !out.mat || !d_num_klns || !d_num_slns || !d_ws)
    return fail(LINETR_E_ARG, "fixed_size: null pointer");
  if (clip_height <= 0) clip_height = height;
  if (clip_width <= 0) clip_width = width;
  if (pseudo_clip_height <= 0) pseudo_clip_height = height;
  if (pseudo_clip_width <= 0) pseudo_clip_width = width;
  if (h_cu_k[0] != 0 || h_cu_n[0] != 0 || h_cu_p[0] != 0) return fail(LINETR_E_ARG, "fixed_size: prefix sums must start at 0");
  for (int b = 0; b < B; ++b) {
    const int64_t nk = (int64_t)h_cu_k[b + 1] - h_cu_k[b], ns = (int64_t)h_cu_n[b + 1] - h_cu_n[b], np = (int64_t)h_cu_p[b + 1] - h_cu_p[b];
    if (nk < 0 || ns < nk || np < 0) return fail(LINETR_E_ARG, "fixed_size: image %d: prefix sums must ascend, with at least one sub-line per key-line", b);
    if (nk > M)
      return fail(LINETR_E_ARG, "fixed_size: image %d has %lld key-lines, more than max_sublines = %d (the reference raises there)", b, (long long)nk, M);
    const int64_t n_add = std::max<int64_t>(M - ns, 0);
    if (np != n_add) return fail(LINETR_E_ARG, "fixed_size: image %d needs %lld pseudo lines, got %lld", b, (long long)n_add, (long long)np);
    if (np > 0 && !h_pseudo) return fail(LINETR_E_ARG, "fixed_size: null pointer");
    for (int64_t p = h_cu_p[b]; p < h_cu_p[b + 1]; ++p) {
      const LinetrLineRec& r = h_pseudo[p];
      if (r.n_sub != 1 || r.n_tok < 1 || r.n_tok > T)
        return fail(LINETR_E_ARG, "fixed_size: pseudo line %lld of image %d makes %d sub-lines (%d tokens), every one must make exactly one",
                    (long long)(p - h_cu_p[b]), b, r.n_sub, r.n_tok);
      if (r.image != b || r.line_local != p - h_cu_p[b]) return fail(LINETR_E_ARG, "fixed_size: pseudo record %lld is not line %lld of image %d", (long long)p, (long long)(p - h_cu_p[b]), b);
    }
  }
  if ((h_cu_k[B] > 0 && !d_recs) || (h_cu_p[B] > 0 && !d_pseudo)) return fail(LINETR_E_ARG, "fixed_size: null pointer");
  if ((dense_is_nhwc && !aligned16(d_dense_desc)) || !aligned16(out.desc) || !aligned16(d_ws))
    return fail(LINETR_E_ARG, "fixed_size: a channel-last descriptor map, out.desc and the workspace must be 16-byte aligned");
  const FsLayout L = fs_layout(B, height, width, dense_is_nhwc);
  if (ws_bytes < L.total) return fail(LINETR_E_WORKSPACE, "fixed_size: workspace too small (need %lld)", (long long)L.total);
  hipStream_t st = (hipStream_t)stream;
  if (h) LT_HIP(hipSetDevice(h->device));
  FsImage* table = (FsImage*)((char*)d_ws + L.o_table);
  for (int first = 0; first < B; first += FS_TABLE_CHUNK) {
    FsChunk c{};
    const int count = std::min(FS_TABLE_CHUNK, B - first);
    for (int i = 0; i < count; ++i) {
      const int b = first + i;
      c.img[i] = FsImage{h_cu_k[b], h_cu_k[b + 1] - h_cu_k[b], h_cu_n[b], h_cu_n[b + 1] - h_cu_n[b], h_cu_p[b], h_cu_p[b + 1] - h_cu_p[b]};
    }
    hipLaunchKernelGGL(fs_table_kernel, dim3(1), dim3(64), 0, st, c, first, count, table);
    LT_LAUNCH_CHECK();
  }
  const int Hc = height / 8, Wc = width / 8;
  const int64_t rows = (int64_t)B * M, ntok = rows * T;
  {
    ProfScope ps(h, st, "fixed_size_rows", 0, (double)rows * (T * 16.0 + M * 4.0 + 64.0));
    hipLaunchKernelGGL(fs_rows_kernel, dim3((unsigned)rows), dim3(64), 0, st, d_recs, d_pseudo, table, M, td, T, height, width,
                       (double)clip_width - 0.6, (double)clip_height - 0.6, (double)pseudo_clip_width - 0.6, (double)pseudo_clip_height - 0.6,
                       d_dense_score, out.klines, out.length, out.angles, out.sublines, out.pnt, out.mask, out.resp, out.angle_sub, out.score,
                       out.mat, d_num_klns, d_num_slns);
    LT_LAUNCH_CHECK();
  }
  const float* nhwc = d_dense_desc;
  if (!dense_is_nhwc) {
    float* buf = (float*)((char*)d_ws + L.o_nhwc);
    ProfScope ps(h, st, "nchw_to_nhwc", 0, 2.0 * B * Hc * Wc * D * 4);
    hipLaunchKernelGGL(nchw_to_nhwc_kernel, dim3(cdiv(Hc * Wc, 64), D / 64, B), dim3(256), 0, st, d_dense_desc, buf, D, Hc * Wc);
    LT_LAUNCH_CHECK();
    nhwc = buf;
  }
  {
    ProfScope ps(h, st, "fixed_size_desc", 0, (double)ntok * D * 4 * 2);
    hipLaunchKernelGGL(fs_sample_kernel, dim3((unsigned)((ntok + 3) / 4)), dim3(256), 0, st, out.pnt, ntok, (int64_t)M * T, nhwc, Hc, Wc,
                       align_corners, out.desc);
    LT_LAUNCH_CHECK();
  }
  return LINETR_OK;
}

// =============================================================================================
// the Adam step and the gradient norm over a table of tensors (lt_adam.h)
// =============================================================================================

namespace {
constexpr int AD_MAX_TENSORS = 65536;
constexpr int64_t AD_MAX_CHUNKS = (int64_t)1 << 30;      // one block a chunk: the grid, and gn_final_kernel's int run bounds
// chunks of any table of n_tensors tensors with n_total elements in all, at most
int64_t ad_chunk_bound(int n_tensors, int64_t n_total) { return n_total / AD_CHUNK + n_tensors; }
bool ad_dims_ok(int n_tensors, int64_t n_total) {
  return n_tensors >= 1 && n_tensors <= AD_MAX_TENSORS && n_total >= 0 && n_total / AD_CHUNK <= AD_MAX_CHUNKS - AD_MAX_TENSORS;
}
// workspace: the table | the chunk prefix [n_tensors + 1] | (the norm alone) one float64 a chunk
struct AdamWsLayout { int64_t o_table, o_prefix, o_partial, total; };
AdamWsLayout adam_ws_layout(int n_tensors, int64_t partials) {
  AdamWsLayout L{};
  Carve c;
  L.o_table = c.take((int64_t)n_tensors * (int64_t)sizeof(LinetrAdamTensor));
  L.o_prefix = c.take(((int64_t)n_tensors + 1) * 4);
  L.o_partial = c.take(partials * 8);
  L.total = c.o + 256;
  return L;
}

// The refusals both entry points share, for `who`, every one before the first launch; `all`: the step reads p, g, m and v, the norm g
// alone.  Leaves the table's chunk count in *chunks.
int adam_table_check(const char* who, const LinetrAdamTensor* tab, int n_tensors, bool all, int64_t* chunks) {
  if (!tab) return fail(LINETR_E_ARG, "%s: null table", who);
  if (n_tensors < 1 || n_tensors > AD_MAX_TENSORS) return fail(LINETR_E_ARG, "%s: %d tensors (1 .. %d)", who, n_tensors, AD_MAX_TENSORS);
  int64_t total = 0;
  for (int t = 0; t < n_tensors; ++t) {
    const LinetrAdamTensor& e = tab[t];
    if (e.n < 0) return fail(LINETR_E_ARG, "%s: tensor %d has n = %lld", who, t, (long long)e.n);
    if (e.n == 0) continue;
    const void* ptrs[4] = {e.g, e.p, e.m, e.v};
    const int used = all ? 4 : 1;
    for (int i = 0; i < used; ++i) {
      if (!ptrs[i] || !aligned4(ptrs[i])) return fail(LINETR_E_ARG, "%s: tensor %d has a NULL or misaligned pointer (4-byte alignment)", who, t);
      for (int j = 0; j < i; ++j)
        if (ptrs[i] == ptrs[j]) return fail(LINETR_E_ARG, "%s: two of tensor %d's pointers are equal", who, t);
    }
    if (all && !std::isfinite(e.step_size)) return fail(LINETR_E_ARG, "%s: tensor %d has step_size %g (finite)", who, t, e.step_size);
    if (all && !(e.bc2_sqrt > 0.f && e.bc2_sqrt <= 1.f)) return fail(LINETR_E_ARG, "%s: tensor %d has bc2_sqrt %g (0 < . <= 1)", who, t, e.bc2_sqrt);
    total += (e.n + AD_CHUNK - 1) / AD_CHUNK;
    if (total > AD_MAX_CHUNKS) return fail(LINETR_E_ARG, "%s: more than 2^30 chunks of %d elements", who, AD_CHUNK);
  }
  *chunks = total;
  return LINETR_OK;
}
int adam_ws_check(const char* who, const void* d_ws, int64_t ws_bytes, int64_t need) {
  if (!d_ws || ((uintptr_t)d_ws & 255)) return fail(LINETR_E_ARG, "%s: the workspace is NULL or not 256-byte aligned", who);
  if (ws_bytes < need) return fail(LINETR_E_ARG, "%s: workspace too small (need %lld)", who, (long long)need);
  return LINETR_OK;
}
// the table and its chunk prefix into the workspace, AD_PIECE entries a launch, through the kernel arguments (lt_adam.h)
int adam_table_upload(hipStream_t st, const LinetrAdamTensor* tab, int n_tensors, LinetrAdamTensor* d_table, int32_t* d_prefix) {
  AdamTablePiece piece;
  int32_t at = 0;
  for (int first = 0; first < n_tensors; first += AD_PIECE) {
    const int count = std::min(AD_PIECE, n_tensors - first);
    for (int i = 0; i < count; ++i) {
      piece.entry[i] = tab[first + i];
      piece.prefix[i] = at;
      at += (int32_t)((tab[first + i].n + AD_CHUNK - 1) / AD_CHUNK);
    }
    piece.prefix[count] = at;
    hipLaunchKernelGGL(ad_table_kernel, dim3(1), dim3(AD_PIECE), 0, st, piece, first, count, (int)(first + count == n_tensors), d_table, d_prefix);
    LT_LAUNCH_CHECK();
  }
  return LINETR_OK;
}
}  // namespace

extern "C" int64_t linetr_adam_workspace_bytes(int32_t n_tensors, int64_t n_total) {
  return ad_dims_ok(n_tensors, n_total) ? adam_ws_layout(n_tensors, 0).total : 0;
}

extern "C" int64_t linetr_grad_norm_workspace_bytes(int32_t n_tensors, int64_t n_total) {
  return ad_dims_ok(n_tensors, n_total) ? adam_ws_layout(n_tensors, ad_chunk_bound(n_tensors, n_total)).total : 0;
}

extern "C" int linetr_adam_step(LinetrHandle* h, const LinetrAdamTensor* h_table, int32_t n_tensors, const LinetrAdamHyper* hyper,
                                const float* d_grad_scale, void* d_ws, int64_t ws_bytes, void* stream) {
  // every refusal comes before the first launch
  int64_t chunks = 0;
  if (int e = adam_table_check("adam_step", h_table, n_tensors, true, &chunks)) return e;
  if (!hyper) return fail(LINETR_E_ARG, "adam_step: null hyper-parameters");
  if (!(hyper->beta1 >= 0.0 && hyper->beta1 < 1.0) || !(hyper->beta2 >= 0.0 && hyper->beta2 < 1.0))
    return fail(LINETR_E_ARG, "adam_step: betas %g / %g (0 <= beta < 1)", hyper->beta1, hyper->beta2);
  if (!(hyper->eps >= 0.0) || !std::isfinite(hyper->eps) || !(hyper->weight_decay >= 0.0) || !std::isfinite(hyper->weight_decay))
    return fail(LINETR_E_ARG, "adam_step: eps %g, weight_decay %g (finite, not negative)", hyper->eps, hyper->weight_decay);
  if (hyper->decoupled != 0 && hyper->decoupled != 1) return fail(LINETR_E_ARG, "adam_step: decoupled %d (0 or 1)", hyper->decoupled);
  if (hyper->decoupled && !std::isfinite(hyper->lr)) return fail(LINETR_E_ARG, "adam_step: lr %g (decoupled weight decay multiplies by 1 - lr wd)", hyper->lr);
  if (!aligned4(d_grad_scale)) return fail(LINETR_E_ARG, "adam_step: misaligned grad scale");
  if (int e = adam_ws_check("adam_step", d_ws, ws_bytes, adam_ws_layout(n_tensors, 0).total)) return e;
  if (chunks == 0) return LINETR_OK;
  AdamK k{};
  k.b1c = (float)(1.0 - hyper->beta1);
  k.b2c = (float)(1.0 - hyper->beta2);
  k.b2 = (float)hyper->beta2;
  k.eps = (float)hyper->eps;
  k.wd = (float)hyper->weight_decay;
  k.decay = (float)(1.0 - hyper->lr * hyper->weight_decay);
  k.mode = hyper->weight_decay != 0.0 ? (hyper->decoupled ? 2 : 1) : 0;
  const AdamWsLayout W = adam_ws_layout(n_tensors, 0);
  LinetrAdamTensor* d_table = (LinetrAdamTensor*)((char*)d_ws + W.o_table);
  int32_t* d_prefix = (int32_t*)((char*)d_ws + W.o_prefix);
  hipStream_t st = (hipStream_t)stream;
  if (h) LT_HIP(hipSetDevice(h->device));
  if (int e = adam_table_upload(st, h_table, n_tensors, d_table, d_prefix)) return e;
  ProfScope ps(h, st, "adam_step", 0, 28.0 * AD_CHUNK * (double)chunks);
  hipLaunchKernelGGL(ad_step_kernel, dim3((unsigned)chunks), dim3(AD_THREADS), 0, st, (const LinetrAdamTensor*)d_table, (const int32_t*)d_prefix,
                     (int)n_tensors, k, d_grad_scale);
  LT_LAUNCH_CHECK();
  return LINETR_OK;
}

extern "C" int linetr_grad_norm(LinetrHandle* h, const LinetrAdamTensor* h_table, int32_t n_tensors, double max_norm, double* d_norm,
                                float* d_scale, void* d_ws, int64_t ws_bytes, void* stream) {
  int64_t chunks = 0;
  if (int e = adam_table_check("grad_norm", h_table, n_tensors, false, &chunks)) return e;
  if (!(max_norm >= 0.0)) return fail(LINETR_E_ARG, "grad_norm: max_norm %g (not negative; +inf for the norm alone)", max_norm);
  if (!d_norm || !d_scale || ((uintptr_t)d_norm & 7) || !aligned4(d_scale)) return fail(LINETR_E_ARG, "grad_norm: NULL or misaligned d_norm / d_scale");
  if (int e = adam_ws_check("grad_norm", d_ws, ws_bytes, adam_ws_layout(n_tensors, chunks).total)) return e;
  const AdamWsLayout W = adam_ws_layout(n_tensors, chunks);
  LinetrAdamTensor* d_table = (LinetrAdamTensor*)((char*)d_ws + W.o_table);
  int32_t* d_prefix = (int32_t*)((char*)d_ws + W.o_prefix);
  double* partial = (double*)((char*)d_ws + W.o_partial);
  hipStream_t st = (hipStream_t)stream;
  if (h) LT_HIP(hipSetDevice(h->device));
  if (chunks > 0) {
    if (int e = adam_table_upload(st, h_table, n_tensors, d_table, d_prefix)) return e;
    ProfScope ps(h, st, "grad_norm_partial", 0, 4.0 * AD_CHUNK * (double)chunks);
    hipLaunchKernelGGL(gn_partial_kernel, dim3((unsigned)chunks), dim3(AD_THREADS), 0, st, (const LinetrAdamTensor*)d_table,
                       (const int32_t*)d_prefix, (int)n_tensors, partial);
    LT_LAUNCH_CHECK();
  }
  ProfScope ps(h, st, "grad_norm_final", 0, 8.0 * (double)chunks);      // (no element at all: norm 0, scale 1)
  hipLaunchKernelGGL(gn_final_kernel, dim3(1), dim3(AD_THREADS), 0, st, (const double*)partial, (int)chunks, max_norm, d_norm, d_scale);
  LT_LAUNCH_CHECK();
  return LINETR_OK;
}
