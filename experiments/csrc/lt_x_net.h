// Experiments build only (liblinetr_hip_experiments.so): everything the experiments add to the forward pass.  linetr_net.hip
// includes this file textually, behind sig_network: lt_st_image.h, lt_model.h and lt_attn.h define non-template kernels, so a second
// translation unit would duplicate their host stubs, and the code here uses that file's local helpers (run_gemm, NormSpec,
// FwdWs, TokenStage, sentence, sig_attention, pipe_boundary).  The hooks linetr_net.hip calls:
//   x_gemm           run_gemm: the stream-K tail (LINETR_STREAMK) and the row-owner GEMM (LINETR_GEMM_RO) take the launch
//   x_split_weights  make_split_copies: an ST image of every eligible weight, and each signature layer's W2p
//   x_ws_bytes       fwd_layout: the split-tile activation images and the pairnet area, carved from FwdWs::x
//   x_begin          forward_core, before the encoders: zeroes the pairnet counters and chooses the path (XPath)
//   x_rest           forward_core, behind cls_pooling: the sentence rows and the signature network of the chosen path
#pragma once
#include "lt_gemm_sk.h"
#include "lt_gemm_st.h"
#include "lt_gemm_ro.h"
#include "lt_gemm_chain.h"
#include "lt_mlp_fused.h"
#include "lt_attn_st.h"
#include "lt_pairnet_host.h"

namespace {

int x_gemm(LinetrHandle* h, hipStream_t st, SplitGemmArgs& sa, const GemmW& w, int groups, const NormSpec* fused_norm,
           double fl, double by, bool& done) {
  const GemmArgs& g = sa.g;
  // row-owner kernel (lt_gemm_ro.h): 4-wave blocks, two per CU, operands by LDS-DMA.  Measured at cfg3: 117 TF-eq against 137 for
  // the register-staged tiles (a two-slot ring leaves a DMA one K step to land, and the barrier comes every 48 MFMAs), so opt-in.
  if (h->precision == LINETR_PREC_BF16X6 && LT_XENV("LINETR_GEMM_RO") != nullptr && groups == 1 && g.N % 256 == 0 && g.K % 32 == 0 &&
      w.st && g.lda % 4 == 0 && g.ldy % 4 == 0 && (!g.A2 || (g.lda2 % 4 == 0 && g.K1 % 16 == 0)) && (!g.R || g.ldr % 4 == 0) &&
      g.act != ACT_DIST && cdiv(g.M, 128) * (g.N / 256) >= 140) {
    RoGemmArgs a;
    a.A1 = g.A; a.lda1 = g.lda; a.nk1 = (g.A2 ? g.K1 : g.K) / 16; a.A2 = g.A2; a.lda2 = g.lda2; a.nk2 = g.A2 ? (g.K - g.K1) / 16 : 0;
    a.Wst = w.st; a.bias = g.bias ? g.bias : h->zeros; a.R = g.R; a.ldr = g.ldr; a.Y = g.Y; a.ldy = g.ldy;
    a.M = g.M; a.N = g.N; a.act = g.act;
    if (fused_norm) { a.norm = fused_norm->mode; a.gamma = fused_norm->gamma; a.beta = fused_norm->beta; a.add2 = fused_norm->add2; a.ldadd2 = D; a.eps = fused_norm->eps; }
    done = true;
    ProfScope ps(h, st, "gemm_bf16x6_ro128x256", fl, by);
    return gemm_ro_launch(a, st);
  }
  // stream-K tail (lt_gemm_sk.h), opt-in, behind the row-owner GEMM as before: takes the launches run_gemm would give to the 128x256 tile when a tail pays; a shape
  // that tile refuses is left to gemm_split_launch to refuse.  The 32 MB workspace is only allocated when it is first needed.
  SplitTile tile = SplitTile::count;
  if (LT_XENV("LINETR_STREAMK") && !gemm_ws_takes(h, g, w, groups, fused_norm))
    if (int e = pick_split_tile(g, groups, h->precision == LINETR_PREC_BF16X6 ? 3 : 2, tile)) return e;
  if (tile == SplitTile::t128x256 && g.N % 256 == 0 && g.K % 32 == 0 && (!g.A2 || g.K1 % 32 == 0) && (g.norm == 0 || g.N == 256) &&
      gemm_split_sk_pays(g, groups)) {
    if (!h->sk_ws) {
      constexpr size_t slots = 256, slot_bytes = 128 * 256 * sizeof(float);
      LT_HIP(hipMalloc((void**)&h->sk_ws, slots * slot_bytes));
      LT_HIP(hipMalloc((void**)&h->sk_flags, (slots + 1) * sizeof(unsigned)));
      LT_HIP(hipMemset(h->sk_flags, 0, (slots + 1) * sizeof(unsigned)));
      LT_HIP(hipDeviceSynchronize());
    }
    done = true;
    ProfScope ps(h, st, gemm_class_name(h->precision, (int)tile, g, groups), fl, by);
    switch (h->precision) {
      case LINETR_PREC_BF16X3: sa.Wsp = w.s2; return gemm_split_sk_launch<2, 0>(sa, h->sk_ws, h->sk_flags, ++h->sk_epoch, st);
      case LINETR_PREC_F16X3: sa.Wsp = w.h2; return gemm_split_sk_launch<2, 1>(sa, h->sk_ws, h->sk_flags, ++h->sk_epoch, st);
      default: sa.Wsp = w.s3; return gemm_split_sk_launch<3, 0>(sa, h->sk_ws, h->sk_flags, ++h->sk_epoch, st);
    }
  }
  return LINETR_OK;
}

// Every eligible weight gets an ST image (the ST and row-owner GEMMs read them), and each signature layer's W2 a copy W2p with K
// permuted inside 16-groups, whose split planes the fused signature MLP reads (lt_mlp_fused.h).  Same fp32 values as S.W2.
int x_split_weights(LinetrHandle* H, std::vector<GemmWSpec>& weights) {
  for (auto& w : weights) w.st = true;
  if (H->sig.empty()) return LINETR_OK;
  const size_t n = (size_t)D * 2 * D;
  LT_HIP(hipMalloc((void**)&H->w2p_arena, H->sig.size() * n * sizeof(float)));
  std::vector<float> w2(n), w2p(n);
  for (size_t l = 0; l < H->sig.size(); ++l) {
    SigLayer& S = H->sig[l];
    LT_HIP(hipMemcpy(w2.data(), S.W2.W, n * sizeof(float), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i) w2p[i] = w2[sig_mlp_kperm((int)i)];   // (rows of 2 D: the permutation stays inside a row)
    float* dst = H->w2p_arena + l * n;
    LT_HIP(hipMemcpy(dst, w2p.data(), n * sizeof(float), hipMemcpyHostToDevice));
    S.W2p.W = dst; S.W2p.b = S.W2.b; S.W2p.rows = D; S.W2p.K = 2 * D;
    weights.push_back({&S.W2p, true});
  }
  return LINETR_OK;
}

// ---- the experiments' share of the forward workspace, from FwdWs::x
struct XWs {
  unsigned char *zsA, *zsB, *qkvs, *msgs, *hids;   // split-tile images of the signature network's activations (lt_gemm_st.h)
  char* pn;                                        // activations + arrival counters of the single-pair persistent network (lt_pairnet.h)
  int64_t total;
};
XWs x_layout(const LinetrHandle* h, int N, char* x) {
  XWs s;
  const int64_t pad = -(intptr_t)x & 1023;         // the ST images start on a 1024-byte boundary
  int64_t off = pad;
  auto take_st = [&](int cols) { unsigned char* p = (unsigned char*)(x + off); off += align_up(st_bytes(N, cols), 1024); return p; };
  s.zsA = take_st(D); s.zsB = take_st(D); s.qkvs = take_st(3 * D); s.msgs = take_st(D); s.hids = take_st(2 * D);
  s.pn = x + off;
  s.total = 1024 + (off - pad) + pairnet_ws_bytes(h, N);   // (room for any pad; pairnet_ws_bytes is 0 for batches the path does not take)
  return s;
}

int64_t x_ws_bytes(const LinetrHandle* h, int N) { return x_layout(h, N, nullptr).total; }

// ---- row-tile-local GEMM chains (lt_gemm_chain.h) ----------------------------------------------------------------
struct ChainBuilder {
  LinetrHandle* h;
  ChainArgs c;
  double flops = 0, bytes = 0;
  int err = 0;
  explicit ChainBuilder(LinetrHandle* h_) : h(h_) {}
  // Y[M,N] = norm(act(A (| A2) W^T + bias) (+ R)) (+ add2), Y and R with row stride N
  void add(const GemmW& w, int M, const GemmA& A, float* Y, int act, const float* R = nullptr, const NormSpec* ns = nullptr) {
    if (err) return;
    if (c.n >= CHAIN_MAX) { err = fail(LINETR_E_ARG, "gemm chain: too many stages"); return; }
    SplitGemmArgs& sa = c.st[c.n++];
    sa = SplitGemmArgs{};
    GemmArgs& g = sa.g;
    if ((err = gemm_args(w, M, A, {Y, w.rows}, act, R, nullptr, ns, g))) return;
    sa.Wsp = w.s3;
    sa.wide_epi = 1;
    flops += 2.0 * M * (double)g.N * g.K;
    bytes += 4.0 * ((double)M * g.K + (double)g.N * g.K + (double)M * g.N);
  }
  int run(hipStream_t st, const char* name) {
    if (err) return err;
    ProfScope ps(h, st, name, flops, bytes);
    return gemm_chain_launch(c, st);
  }
};

// A chain is one block per 128-row tile for the WHOLE chain: worth it when the row tiles fill the chip in one round (the
// partly empty second round of a plain launch would be a whole chain long) or there are many rounds.
bool chain_wins(const LinetrHandle* h, int rows) {
  // opt-in (read per call): measured at cfg3, 2.70 vs 2.60 ms per step -- a chain keeps 199 of the 256 CUs busy for all of its
  // stages and the per-tile prologue / epilogue cost, not the launch, is what a GEMM of this size pays
  if (LT_XENV("LINETR_GEMM_CHAIN") == nullptr || h->precision != LINETR_PREC_BF16X6) return false;
  const int gy = cdiv(rows, 128);
  return (gy >= 140 && gy <= cu_count()) || gy >= 4 * cu_count();
}

// the descriptive layer's tail as a chain: [fc + LN] -> [w_1, GELU] -> [w_2 + residual + LN (+ line position)] -> [q/k/v of
// signature layer 0], one launch
int sentence_chain(LinetrHandle* h, hipStream_t st, int N, FwdWs& w) {
  const LinetrModelConfig& c = h->cfg;
  ChainBuilder cb(h);
  NormSpec ns1; ns1.mode = 1; ns1.gamma = h->ln1g; ns1.beta = h->ln1b; ns1.eps = 1e-6f;
  NormSpec ns2; ns2.mode = 1; ns2.gamma = h->ln2g; ns2.beta = h->ln2b; ns2.add2 = w.lpos; ns2.eps = 1e-6f;
  cb.add(h->Wfc, N, {w.att, D}, w.o, ACT_NONE, nullptr, &ns1);
  cb.add(h->Wf1, N, {w.o, D}, w.f1, ACT_GELU);
  cb.add(h->Wf2, N, {w.f1, c.d_inner}, w.zA, ACT_NONE, w.o, &ns2);
  cb.add(h->sig[0].Wqkv, N, {w.zA, D}, w.qkv, ACT_NONE);
  return cb.run(st, "gemm_chain_bf16x6_cls");
}

// the signature network as chains: attention, then W1 -> W2 + residual -> the NEXT layer's q/k/v projection in one launch; the
// last layer W1 -> [final projection with W2 folded in] -> L2 normalisation
int sig_network_chain(LinetrHandle* h, hipStream_t st, const int32_t* h_cu, const int* cu_dev, int n_images, int N, int max_n,
                      float* d_line_desc, FwdWs& w) {
  const double attn_fl = attn_flops(h_cu, n_images);
  const int attn_kernel = sig_attn_plan(h, n_images, N, max_n).attn;
  float *z = w.zA, *zn = w.zB;
  int e;
  for (size_t l = 0;; ++l) {
    const SigLayer& S = h->sig[l];
    // (q/k/v: the previous chain has made them)
    if ((e = sig_attention(h, st, attn_kernel, w.qkv, 3 * D, cu_dev, n_images, N, max_n, attn_fl, w.msgp))) return e;
    ChainBuilder cb(h);
    const bool w1_alone = LT_XENV("LINETR_CHAIN_W1_ALONE") != nullptr;     // A/B: W1 as its own launch (all 256 CUs)
    if (w1_alone && l + 1 < h->sig.size()) {
      if ((e = run_gemm(h, st, S.W1, N, {z, D, w.msgp, D, D}, {w.hid, 2 * D}, ACT_RELU))) return e;
    } else
    cb.add(S.W1, N, {z, D, w.msgp, D, D}, w.hid, ACT_RELU);
    if (l + 1 == h->sig.size()) {
      NormSpec nl2; nl2.mode = 2;
      cb.add(h->Wfin2, N, {z, D, w.hid, 2 * D, D}, d_line_desc, ACT_NONE, nullptr, &nl2);
      return cb.run(st, "gemm_chain_bf16x6_final");
    }
    cb.add(S.W2, N, {w.hid, 2 * D}, zn, ACT_NONE, z);
    cb.add(h->sig[l + 1].Wqkv, N, {zn, D}, w.qkv, ACT_NONE);
    if ((e = cb.run(st, "gemm_chain_bf16x6_sig"))) return e;
    std::swap(z, zn);
  }
}

// ---- fused signature MLP (lt_mlp_fused.h): z' = z + W2 relu(W1 [z ; msg] + b1) + b2 in one launch (split-bf16 modes only)
int run_sig_mlp(LinetrHandle* h, hipStream_t st, const float* z, const float* msg, const SigLayer& S, float* out, int M) {
  SigMlpArgs a;
  a.z = z; a.ldz = D; a.msg = msg; a.ldm = D; a.b1 = S.W1.b; a.b2 = S.W2.b; a.out = out; a.ldo = D; a.M = M;
  const double fl = 2.0 * M * (2.0 * D * 2 * D + 2.0 * D * D), by = 4.0 * M * 3.0 * D;
  if (h->precision == LINETR_PREC_BF16X3) {
    a.W1sp = S.W1.s2; a.W2sp = S.W2p.s2;
    ProfScope ps(h, st, "sig_mlp_bf16x3", fl, by);
    if (int e = sig_mlp_fused_launch<2, 0>(a, st)) return e;
  } else if (h->precision == LINETR_PREC_F16X3) {
    a.W1sp = S.W1.h2; a.W2sp = S.W2p.h2;
    ProfScope ps(h, st, "sig_mlp_f16x3", fl, by);
    if (int e = sig_mlp_fused_launch<2, 1>(a, st)) return e;
  } else {
    a.W1sp = S.W1.s3; a.W2sp = S.W2p.s3;
    ProfScope ps(h, st, "sig_mlp_bf16x6", fl, by);
    if (int e = sig_mlp_fused_launch<3, 0>(a, st)) return e;
  }
  LT_LAUNCH_CHECK();
  return 0;
}

// sig_network with the fused MLP in every layer but the last (N >= 4096: neither fold_next nor the small attention applies)
int sig_network_fused_mlp(LinetrHandle* h, hipStream_t st, const TokenStage& ts, const int32_t* h_cu, const int* cu_dev, int n_images,
                          int N, int max_n, float* d_line_desc, FwdWs& w) {
  const LinetrModelConfig& c = h->cfg;
  const double attn_fl = attn_flops(h_cu, n_images);
  const int64_t sig_bn_off = 4 * (int64_t)(c.enc_channels[0] + c.enc_channels[1] + c.enc_channels[2] + c.enc_channels[3]);
  const int attn_kernel = sig_attn_plan(h, n_images, N, max_n).attn;
  const bool fused_qkv_attn = !LT_XENV("LINETR_NO_FUSED_QKV_ATTN") && h->precision == LINETR_PREC_BF16X6 && max_n <= 256 &&
                              (int64_t)n_images * HEADS >= 128;
  float *z = w.zA, *zn = w.zB;
  int e;
  for (size_t l = 0;; ++l) {
    const SigLayer& S = h->sig[l];
    if (fused_qkv_attn && S.Wqkv.st) {
      if ((e = sig_qkv_attention(h, st, S, z, cu_dev, n_images, N, max_n, false, attn_fl, w.msgp))) return e;
    } else {
      if ((e = run_gemm(h, st, S.Wqkv, N, {z, D}, {w.qkv, 3 * D}, ACT_NONE))) return e;
      if ((e = sig_attention(h, st, attn_kernel, w.qkv, 3 * D, cu_dev, n_images, N, max_n, attn_fl, w.msgp))) return e;
    }
    if (l + 1 == h->sig.size()) break;
    if ((e = run_sig_mlp(h, st, z, w.msgp, S, zn, N))) return e;
    std::swap(z, zn);
  }
  const size_t l = h->sig.size() - 1;
  if ((e = run_gemm(h, st, h->sig[l].W1, N, {z, D, w.msgp, D, D}, {w.hid, 2 * D}, ts.bn ? ACT_NONE : ACT_RELU))) return e;
  if (ts.bn && (e = bn_train_layer(st, *ts.bn, w.hid, N, 2 * D, 2 * D, h->bn_g[8 + l], h->bn_b[8 + l], sig_bn_off + (int64_t)l * 4 * D))) return e;
  NormSpec l2; l2.mode = 2;
  return run_gemm_norm(h, st, h->Wfin2, N, {z, D, w.hid, 2 * D, D}, nullptr, zn, d_line_desc, l2);
}

// ---- split-tile signature network (lt_gemm_st.h, lt_attn_st.h)
// Signature network on split-tile operands: z -> [q|k|v] -> attention -> W1 [z ; message] -> W2 + z, seven times, then the
// final projection (with the last W2 folded in) and the L2 normalisation.  models/line_transformer.py:132-183, 245-246.
int sig_network_st(LinetrHandle* h, hipStream_t st, FwdWs& w, const XWs& x, const int32_t* h_cu, const int* cu_dev, int n_images,
                   int N, int max_n, float* d_line_desc) {
  auto gemm = [&](const char* role, const unsigned char* A1, int K1, const unsigned char* A2, int K2, const GemmW& W,
                  const unsigned char* R, unsigned char* Yst, float* Y, int act) -> int {
    const int Nout = W.rows;
    StGemmArgs a;
    a.A1 = A1; a.nk1 = K1 / 16; a.A2 = A2; a.nk2 = A2 ? K2 / 16 : 0;
    a.W = W.st; a.bias = W.b ? W.b : h->zeros; a.R = R; a.Yst = Yst; a.Y = Y; a.ldy = D; a.M = N; a.N = Nout; a.act = act;
    if (!a.W) return fail(LINETR_E_ARG, "sig_network_st: weight has no split-tile image");
    const double K = K1 + (A2 ? K2 : 0);
    ProfScope ps(h, st, role, 2.0 * N * Nout * K, 6.0 * ((double)N * K + (double)Nout * K + (double)N * Nout));
    return gemm_st_launch(a, st);
  };
  if (st_bytes(N, 3 * D) >= (int64_t)1 << 32) return fail(LINETR_E_ARG, "sig_network_st: batch too large (q/k/v image >= 4 GiB)");
  int e;
  {
    ProfScope ps(h, st, "to_st", 0, (double)N * D * 10);
    const int64_t thr = st_row_blocks(N) * (D / 16) * 32;
    hipLaunchKernelGGL(to_st_kernel, dim3((unsigned)((thr + 255) / 256)), dim3(256), 0, st, w.zA, D, N, D / 16, x.zsA);
    LT_LAUNCH_CHECK();
  }
  unsigned char *z = x.zsA, *zn = x.zsB;
  const double attn_fl = attn_flops(h_cu, n_images);
  for (size_t l = 0; l < h->sig.size(); ++l) {
    const SigLayer& S = h->sig[l];
    if ((e = gemm("gemm_st_bf16x6_qkv", z, D, nullptr, 0, S.Wqkv, nullptr, x.qkvs, nullptr, ACT_NONE))) return e;
    {
      ProfScope ps(h, st, "sig_attn_st", attn_fl, (double)N * D * 24);
      const bool occ1 = LT_XENV("LINETR_ATTN_ST_OCC1") != nullptr;   // tuning aid: one block per CU, 256 VGPRs
      if (occ1) hipLaunchKernelGGL(sig_attn_st_kernel<1>, dim3(n_images, HEADS, cdiv(max_n, 256)), dim3(512), 0, st, x.qkvs, cu_dev,
                                   n_images, N, x.msgs);
      else hipLaunchKernelGGL(sig_attn_st_kernel<2>, dim3(n_images, HEADS, cdiv(max_n, 256)), dim3(512), 0, st, x.qkvs, cu_dev,
                              n_images, N, x.msgs);
      LT_LAUNCH_CHECK();
    }
    if ((e = gemm("gemm_st_bf16x6_w1", z, D, x.msgs, D, S.W1, nullptr, x.hids, nullptr, ACT_RELU))) return e;
    if (l + 1 == h->sig.size()) break;   // the last layer's second MLP GEMM is folded into the final projection
    if ((e = gemm("gemm_st_bf16x6_w2", x.hids, 2 * D, nullptr, 0, S.W2, z, zn, nullptr, ACT_NONE))) return e;
    std::swap(z, zn);
  }
  // final_proj(z + W2 hid + b2) = [Wfin | Wfin W2] [z ; hid] + (Wfin b2 + bfin), then F.normalize
  if ((e = gemm("gemm_st_bf16x6_final", z, D, x.hids, 2 * D, h->Wfin2, nullptr, nullptr, w.zB, ACT_NONE))) return e;
  ProfScope ps(h, st, "row_norm", 0, (double)N * D * 8);
  hipLaunchKernelGGL(row_norm_kernel, dim3(cdiv(N, 4)), dim3(256), 0, st, w.zB, N, 1, (const float*)nullptr, (const float*)nullptr,
                     (const float*)nullptr, 0.f, d_line_desc);
  LT_LAUNCH_CHECK();
  return LINETR_OK;
}

// ---- forward_core's hooks
enum XPath { X_NONE, X_CHAIN, X_PAIRNET, X_ST, X_FUSED_MLP };

// before the encoders: which path takes the sentence rows and the signature network (X_NONE: the product's)
int x_begin(LinetrHandle* h, hipStream_t st, int n_images, int N, const int32_t* h_cu, const FwdWs& w, XPath& path) {
  // LINETR_PAIRNET=1 (measured and not shipped): the whole signature network of a single pair as ONE persistent
  // launch (lt_pairnet.h); its arrival counters are zeroed here, far ahead of it on the stream
  const bool pairnet = pairnet_fits(h, n_images, N, h_cu);
  if (pairnet)
    if (int e = pairnet_prepare(h, st, N, x_layout(h, N, w.x).pn)) return e;
  // LINETR_SIG_PATH=st: activations stay in HBM as split-tile images and every K step travels by LDS-DMA (lt_gemm_st.h,
  // lt_attn_st.h).  Measured at cfg3 on one box: the ST GEMMs are 5-7 % faster than the register-staged ones in isolation,
  // but inside the step the 6-byte activations cost more at the kernel boundaries (the L2 write-back of 273 MB instead of
  // 182 MB of fresh activations per layer) than the main loops save: 2.92 vs 2.69 ms per step.
  const char* sig_path = LT_XENV("LINETR_SIG_PATH");      // read per call (tests switch it)
  // LINETR_FUSED_SIG_MLP=1: layers but the last run W1 -> ReLU -> W2 + residual in one kernel, hidden activations in registers
  // (lt_mlp_fused.h).  Measured slower
  const bool fused_sig_mlp = h->precision != LINETR_PREC_F32 && N >= 4096 && !LT_XENV("LINETR_NO_FUSED_SIG_MLP") &&
                             LT_XENV("LINETR_FUSED_SIG_MLP") != nullptr;
  if (h->sig.empty()) path = X_NONE;
  else if (chain_wins(h, N)) path = X_CHAIN;
  else if (pairnet) path = X_PAIRNET;
  else if (h->precision == LINETR_PREC_BF16X6 && sig_path && !strcmp(sig_path, "st")) path = X_ST;
  else if (fused_sig_mlp) path = X_FUSED_MLP;
  else path = X_NONE;
  return LINETR_OK;
}

// behind cls_pooling: the descriptive layer's tail, CUT_SENTENCE and the signature network of `path`.  None of these paths
// cuts the signature network per layer (CUT_SIG0 + l): a pipelined batch stays on the stream it reached at CUT_SENTENCE.
int x_rest(LinetrHandle* h, hipStream_t& st, const TokenStage& ts, const int32_t* h_cu, const int* cu_dev, int n_images, int N,
           float* d_line_desc, FwdWs& w, XPath path) {
  int e;
  if ((e = path == X_CHAIN ? sentence_chain(h, st, N, w) : sentence(h, st, N, w))) return e;
  if ((e = pipe_boundary(ts.pipe, CUT_SENTENCE, st))) return e;
  int max_n = 0;
  for (int i = 0; i < n_images; ++i) max_n = std::max(max_n, h_cu[i + 1] - h_cu[i]);
  const XWs x = x_layout(h, N, w.x);
  switch (path) {
    case X_CHAIN: return sig_network_chain(h, st, h_cu, cu_dev, n_images, N, max_n, d_line_desc, w);
    case X_PAIRNET: return pairnet_run(h, st, w.zA, d_line_desc, h_cu, n_images, N, x.pn);
    case X_ST: return sig_network_st(h, st, w, x, h_cu, cu_dev, n_images, N, max_n, d_line_desc);
    default: return sig_network_fused_mlp(h, st, ts, h_cu, cu_dev, n_images, N, max_n, d_line_desc, w);
  }
}

}  // namespace

// ---- split-tile (ST) format and GEMM (lt_gemm_st.h), for the unit tests and micro-benchmarks
extern "C" int64_t linetr_st_bytes(int64_t rows, int32_t K) { return (K % 16 || rows < 0) ? -1 : st_bytes(rows, K); }

extern "C" int linetr_debug_to_st(LinetrHandle* h, const float* d_X, int32_t ld, int32_t rows, int32_t K, void* d_st,
                                  void* stream) {
  if (!h || !d_X || !d_st || K % 16 || ld < K || ld % 4 || rows < 1) return fail(LINETR_E_ARG, "debug_to_st: bad argument");
  LT_HIP(hipSetDevice(h->device));
  const int64_t thr = st_row_blocks(rows) * (K / 16) * 32;
  hipLaunchKernelGGL(to_st_kernel, dim3((unsigned)((thr + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_X, ld, rows, K / 16,
                     (unsigned char*)d_st);
  LT_LAUNCH_CHECK();
  return LINETR_OK;
}

extern "C" int linetr_debug_from_st(LinetrHandle* h, const void* d_st, int32_t rows, int32_t K, float* d_X, int32_t ld,
                                    void* stream) {
  if (!h || !d_X || !d_st || K % 16 || ld < K || ld % 4 || rows < 1) return fail(LINETR_E_ARG, "debug_from_st: bad argument");
  LT_HIP(hipSetDevice(h->device));
  const int64_t thr = st_row_blocks(rows) * (K / 16) * 32;
  hipLaunchKernelGGL(from_st_kernel, dim3((unsigned)((thr + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (const unsigned char*)d_st, rows, K / 16, d_X, ld);
  LT_LAUNCH_CHECK();
  return LINETR_OK;
}

extern "C" int linetr_debug_gemm_st(LinetrHandle* h, const void* d_A1, int32_t K1, const void* d_A2, int32_t K2,
                                    const void* d_W, const float* d_bias, const void* d_R, void* d_Yst, float* d_Y,
                                    int32_t ldy, int32_t M, int32_t N, int32_t act, void* stream) {
  if (!h || !d_A1 || !d_W || (!d_Yst && !d_Y) || K1 % 16 || K2 % 16 || N > 4096)
    return fail(LINETR_E_ARG, "debug_gemm_st: bad argument");
  LT_HIP(hipSetDevice(h->device));
  StGemmArgs a;
  a.A1 = (const unsigned char*)d_A1; a.nk1 = K1 / 16;
  a.A2 = (const unsigned char*)d_A2; a.nk2 = d_A2 ? K2 / 16 : 0;
  a.W = (const unsigned char*)d_W; a.bias = d_bias ? d_bias : h->zeros; a.R = (const unsigned char*)d_R;
  a.Yst = (unsigned char*)d_Yst; a.Y = d_Y; a.ldy = ldy; a.M = M; a.N = N; a.act = act;
  return gemm_st_launch(a, (hipStream_t)stream);
}
