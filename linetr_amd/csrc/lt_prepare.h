// Weight preparation: the state dict -> the float32 image of the weight arena, in float64 on the host, once per handle.  Every item of
// DESIGN.md section 3 but the padding key is decided here, one function per fold.  Host only: nothing below calls HIP or knows
// LinetrHandle.  linetr_create uploads Prepared::image and points the handle's fields at it entry by entry; linetr_debug_prepare hands
// image and table to tests/test_prepare_cpu.py, which pins every fold to a float64 restatement.  Every sum runs in ascending index order
// from its starting value (the bias, or 0); the image is a function of that order (profiles/prepare_refactor_digest.txt).
#pragma once
#include <algorithm>
#include <map>
#include <numeric>
#include <string>
#include <vector>

#include "lt_common.h"

namespace lt {
using Vec = std::vector<double>;

// ---- float64 helpers ----------------------------------------------------------------------------------------------------------------
template <class T> struct MatT {   // row-major matrix view
  T* p; int rows, cols, ld;
  MatT(T* p_, int rows_, int cols_, int ld_) : p(p_), rows(rows_), cols(cols_), ld(ld_) {}
  template <class V> MatT(V& v, int rows_, int cols_) : MatT(v.data(), rows_, cols_, cols_) {}
  MatT(const MatT<double>& m) : MatT(m.p, m.rows, m.cols, m.ld) {}
  T* row(int r) const { return p + (size_t)r * ld; }
  MatT block(int r0, int c0, int r, int c) const { return MatT(row(r0) + c0, r, c, ld); }
};
using Mat = MatT<double>; using CMat = MatT<const double>;

// C += A B: every element starts at what C holds and takes its terms in ascending m; the inner loop runs along C's row
inline void matmul(Mat C, CMat A, CMat B) {
  for (int r = 0; r < C.rows; ++r) {
    double* __restrict__ c = C.row(r);
    for (int m = 0; m < A.cols; ++m) {
      const double a = A.row(r)[m];
      const double* __restrict__ b = B.row(m);
      for (int j = 0; j < C.cols; ++j) c[j] += a * b[j];
    }
  }
}
// y += A x (y: one element per row of A, `ldy` apart)
inline void matvec(double* y, int ldy, CMat A, const Vec& x) { matmul(Mat(y, A.rows, 1, ldy), A, CMat(x.data(), A.cols, 1, 1)); }
inline double dot(const double* a, const double* b, int n) { return std::inner_product(a, a + n, b, 0.0); }
inline void copy(Mat dst, CMat src) { for (int r = 0; r < src.rows; ++r) std::copy(src.row(r), src.row(r) + src.cols, dst.row(r)); }
// the reference's signature channel c = d * 4 + h (models/line_transformer.py:151) -> head-major c' = h * 64 + d
inline int head_major(int c) { return (c % HEADS) * DH + c / HEADS; }
inline void head_major_rows(Mat dst, CMat src, double scale) {
  for (int c = 0; c < src.rows; ++c)
    for (int i = 0; i < src.cols; ++i) dst.row(head_major(c))[i] = src.row(c)[i] * scale;
}
inline void head_major_cols(Mat dst, CMat src) {
  for (int o = 0; o < src.rows; ++o)
    for (int c = 0; c < src.cols; ++c) dst.row(o)[head_major(c)] = src.row(o)[c];
}

// ---- the state dict -----------------------------------------------------------------------------------------------------------------
struct Affine {   // y = W x + b, W [out, in]
  Vec W, b; int out = 0, in = 0;
  CMat mat() const { return CMat(W, out, in); }
};
struct BatchNorm { Vec g, beta, mean, var; };

// Fetches tensors by name as float64.  A missing or mis-sized tensor sets `err` and the message (the last one of a group stands); the
// caller looks at `err` once per group of fetches, before it reads any of them.
struct TensorMap {
  std::map<std::string, std::pair<const float*, int64_t>> t;
  int err = 0;
  TensorMap(int32_t n_tensors, const char* const* names, const float* const* h_data, const int64_t* numel) {
    for (int i = 0; i < n_tensors; ++i) t[names[i]] = {h_data[i], numel[i]};
  }
  Vec get(const std::string& k, int64_t numel) {
    auto it = t.find(k);
    if (it == t.end() || it->second.first == nullptr) err = fail(LINETR_E_WEIGHTS, "state_dict tensor '%s' missing", k.c_str());
    else if (it->second.second != numel)
      err = fail(LINETR_E_WEIGHTS, "state_dict tensor '%s' has %lld elements, expected %lld", k.c_str(), (long long)it->second.second, (long long)numel);
    else return Vec(it->second.first, it->second.first + numel);
    return {};
  }
  // `.weight` and `.bias` of a convolution / linear layer (a LayerNorm: in = 1)
  Affine conv(const std::string& p, int out, int in) { return {get(p + ".weight", (int64_t)out * in), get(p + ".bias", out), out, in}; }
  BatchNorm bn(const std::string& p, int c) { return {get(p + ".weight", c), get(p + ".bias", c), get(p + ".running_mean", c), get(p + ".running_var", c)}; }
};

// ---- the result: the arena image and its table (entry names: include/linetr_hip.h, linetr_debug_prepare) ------------------------------
// off: floats from the start of the image, a multiple of 64.  gemm: a GEMM weight [rows, K = cols], the entry behind it is its bias; st: it
// also gets a split-tile image (lt_st_image.h)
struct PreparedEntry { std::string name; size_t off; int rows, cols; bool gemm, st; };
struct Prepared {
  std::vector<float> image;
  std::vector<PreparedEntry> table;
  float c_tok[HEADS], s_cls[HEADS];   // the scalar halves of ClsPoolConst
  void put(const std::string& name, const Vec& v, int rows, int cols = 1, bool gemm = false, bool st = false) {
    const size_t off = (image.size() + 63) / 64 * 64;
    image.resize(off + v.size());
    for (size_t i = 0; i < v.size(); ++i) image[off + i] = (float)v[i];
    table.push_back({name, off, rows, cols, gemm, st});
  }
  void put_gemm(const std::string& name, const Affine& a, bool st = false) {
    put(name, a.W, a.out, a.in, true, st);
    put("b" + name.substr(1), a.b, a.out);
  }
};

// ---- the folds --------------------------------------------------------------------------------------------------
// Conv1d(k=1) + BatchNorm1d(eval) -> one affine map (models/line_transformer.py:9-20)
inline void fold_bn(Affine& a, const BatchNorm& n) {
  for (int o = 0; o < a.out; ++o) {
    const double s = n.g[o] / std::sqrt(n.var[o] + 1e-5);
    for (int i = 0; i < a.in; ++i) a.W[(size_t)o * a.in + i] = a.W[(size_t)o * a.in + i] * s;
    a.b[o] = (a.b[o] - n.mean[o]) * s + n.beta[o];
  }
}
// conv + BatchNorm as the handle runs it: folded, or under bn_batch_stats the convolution as it is and gamma / beta in the next slot of
// the packed statistics (BatchNorm applied by lt_bntrain.h)
inline void conv_bn(const LinetrModelConfig& cfg, Prepared& P, int& bn_slot, Affine& a, const BatchNorm& n) {
  if (!cfg.bn_batch_stats) return fold_bn(a, n);
  P.put("bn_g" + std::to_string(bn_slot), n.g, a.out);
  P.put("bn_b" + std::to_string(bn_slot++), n.beta, a.out);
}
// A linear layer behind another, as one map over [x ; y]:  left x + A (inner.W y + inner.b) + b  =  [left | A inner.W] [x ; y] + (b + A inner.b)
// (`pad` zero columns behind)
inline Affine fold_inner(CMat left, CMat A, const Affine& inner, const Vec& b, int pad = 0) {
  Affine f{Vec((size_t)A.rows * (left.cols + inner.in + pad), 0.0), b, A.rows, left.cols + inner.in + pad};
  copy(Mat(f.W, f.out, f.in), left);
  matmul(Mat(f.W, f.out, f.in).block(0, left.cols, f.out, inner.in), A, inner.mat());
  matvec(f.b.data(), 1, A, inner.b);
  return f;
}

// positional encoders: 4 x (conv + BN + ReLU) + linear.  The word encoder's last layer is consumed algebraically: returned, not placed.
inline int pos_encoders(const LinetrModelConfig& cfg, TensorMap& tm, Prepared& P, int& bn_slot, Affine& W5word) {
  for (int enc = 0; enc < 2; ++enc) {
    const std::string name = enc == 0 ? "word" : "line", pre = "klenc." + name + "_position_enc.encoder.";
    const int ch[6] = {enc == 0 ? 3 : 5, cfg.enc_channels[0], cfg.enc_channels[1], cfg.enc_channels[2], cfg.enc_channels[3], D};
    for (int i = 0; i < 4; ++i) {
      Affine a = tm.conv(pre + std::to_string(3 * i), ch[i + 1], ch[i]);
      const BatchNorm n = tm.bn(pre + std::to_string(3 * i + 1), ch[i + 1]);
      if (tm.err) return tm.err;
      conv_bn(cfg, P, bn_slot, a, n);
      // layers 2-4 also get split-tile images: the one-kernel MLP of lt_tokmlp.h keeps layers 2 / 3 in LDS and layer 4 in registers as
      // such, and the weight-stationary GEMM of lt_gemm_ws.h reads layer 4's planes from one
      if (i == 0) { P.put("W" + name + "1", a.W, a.out, a.in); P.put("b" + name + "1", a.b, a.out); }
      else P.put_gemm("W" + name + std::to_string(i + 1), a, true);
    }
    const Affine last = tm.conv(pre + "12", D, cfg.enc_channels[3]);
    if (tm.err) return tm.err;
    if (enc == 0) W5word = last; else P.put_gemm("Wline5", last);
  }
  return 0;
}

// CLS-only pooling: score_hj = u_h . x_j + c_h with u_h = Wk_h^T q_h, c_h = q_h . bk_h and q the CLS query pre-scaled by 1/sqrt(64)
// (line_attention.py:14; the descriptive heads are head-major, :55-57); U2_h = W5^T u_h takes the word encoder's last layer along
inline void pooling_constants(Prepared& P, const Vec& cls, const Affine& Wq, const Affine& Wk, const Affine& W5) {
  Vec q = Wq.b, U(HEADS * D, 0.0), U2(HEADS * D, 0.0);
  matvec(q.data(), 1, Wq.mat(), cls);
  for (double& v : q) v = v / 8.0;
  for (int h = 0; h < HEADS; ++h) {
    const double c = dot(&q[h * DH], &Wk.b[h * DH], DH);
    matmul(Mat(&U[h * D], 1, D, D), CMat(&q[h * DH], 1, DH, DH), Wk.mat().block(h * DH, 0, DH, D));
    matmul(Mat(&U2[h * D], 1, D, D), CMat(&U[h * D], 1, D, D), W5.mat());
    P.c_tok[h] = (float)(dot(&U[h * D], W5.b.data(), D) + c);
    P.s_cls[h] = (float)(dot(&U[h * D], cls.data(), D) + c);
  }
  P.put("U", U, HEADS, D); P.put("U2", U2, HEADS, D);
}

// value path after pooling: att_h = Wv_h dbar + (Wv_h W5) abar + p0 * Wv_h (cls - b5) + (Wv_h b5 + bv_h) over [dbar | abar | p0 | 0]
inline void value_path(Prepared& P, const Vec& cls, const Affine& Wv, const Affine& W5) {
  Affine att = fold_inner(Wv.mat(), Wv.mat(), W5, Wv.b, POOLW - 2 * D);
  Vec cls_b5(D);
  for (int i = 0; i < D; ++i) cls_b5[i] = cls[i] - W5.b[i];
  matvec(&att.W[2 * D], POOLW, Wv.mat(), cls_b5);
  P.put_gemm("Watt", att);
}

// line-descriptive layer: only the last one matters (line_transformer.py:123-125), and of it only the CLS row
inline int descriptive_layer(const LinetrModelConfig& cfg, TensorMap& tm, Prepared& P, const Affine& W5word) {
  const std::string p = "klenc.desc_layers." + std::to_string(cfg.n_desc_layers - 1) + ".";
  const Vec cls = tm.get("klenc.cls_token", D);
  const Affine Wq = tm.conv(p + "slf_attn.w_qs", D, D), Wk = tm.conv(p + "slf_attn.w_ks", D, D), Wv = tm.conv(p + "slf_attn.w_vs", D, D);
  Affine fc = tm.conv(p + "slf_attn.fc", D, D);
  const Affine ln1 = tm.conv(p + "slf_attn.layer_norm", D, 1);
  const Affine f1 = tm.conv(p + "pos_ffn.w_1", cfg.d_inner, D), f2 = tm.conv(p + "pos_ffn.w_2", D, cfg.d_inner);
  const Affine ln2 = tm.conv(p + "pos_ffn.layer_norm", D, 1);
  if (tm.err) return tm.err;
  pooling_constants(P, cls, Wq, Wk, W5word);
  value_path(P, cls, Wv, W5word);
  // fc, LayerNorms and FFN pass through; the residual of the CLS row is the constant token, so it joins the fc bias
  for (int i = 0; i < D; ++i) fc.b[i] = fc.b[i] + cls[i];
  P.put_gemm("Wfc", fc);
  P.put("ln1g", ln1.W, D); P.put("ln1b", ln1.b, D);
  P.put_gemm("Wf1", f1); P.put_gemm("Wf2", f2);
  P.put("ln2g", ln2.W, D); P.put("ln2b", ln2.b, D);
  return 0;
}

// One signature layer.  q/k/v rows to head-major, q scaled by 1/sqrt(64) (line_transformer.py:134, an exact power of two); BatchNorm
// into the MLP's first layer; the attention's merge conv into it as well (both linear, nothing in between):
//   W1 [x ; Wm a + bm] + b1 = W1a x + (W1b Wm) a + (W1b bm + b1)            (line_transformer.py:154,:166)
// Leaves the layer's q/k/v projection and second MLP layer in `qkv` / `W2` for the folds across layers.
inline int signature_layer(const LinetrModelConfig& cfg, TensorMap& tm, Prepared& P, int& bn_slot, int l, Affine& qkv, Affine& W2) {
  const std::string p = "selfattn.layers." + std::to_string(l) + ".", ls = std::to_string(l);
  Affine proj[3];
  for (int j = 0; j < 3; ++j) proj[j] = tm.conv(p + "attn.proj." + std::to_string(j), D, D);
  Affine merge = tm.conv(p + "attn.merge", D, D), W1 = tm.conv(p + "mlp.0", 2 * D, 2 * D);
  const BatchNorm n = tm.bn(p + "mlp.1", 2 * D);
  W2 = tm.conv(p + "mlp.3", D, 2 * D);
  if (tm.err) return tm.err;
  qkv = {Vec((size_t)3 * D * D), Vec(3 * D), 3 * D, D};
  for (int j = 0; j < 3; ++j) {
    head_major_rows(Mat(qkv.W, 3 * D, D).block(j * D, 0, D, D), proj[j].mat(), j == 0 ? 0.125 : 1.0);
    head_major_rows(Mat(qkv.b, 3 * D, 1).block(j * D, 0, D, 1), CMat(proj[j].b, D, 1), j == 0 ? 0.125 : 1.0);
  }
  const Vec Wm = merge.W;
  head_major_cols(Mat(merge.W, D, D), CMat(Wm, D, D));
  conv_bn(cfg, P, bn_slot, W1, n);
  P.put_gemm("Wqkv" + ls, qkv, true);
  P.put_gemm("W1m" + ls, fold_inner(W1.mat().block(0, 0, 2 * D, D), W1.mat().block(0, D, 2 * D, D), merge, W1.b));
  P.put_gemm("W2" + ls, W2);
  return 0;
}

// x_out = z + W2 hid + b2 (line_transformer.py:180-183) and the next layer's q/k/v projection is linear in x_out (:141-143), so
//   [x_out ; qkv_next] = [[I, W2], [Wqkv, Wqkv W2]] [z ; hid] + [b2 ; Wqkv b2 + bqkv]
// one contraction instead of two dependent ones -- 2.4x the flops, which only pays at single-pair sizes (linetr_net.hip)
inline void wnext(Prepared& P, int l, const Affine& W2, const Affine& qkv_next) {
  const Affine low = fold_inner(qkv_next.mat(), qkv_next.mat(), W2, qkv_next.b);
  Affine a{Vec((size_t)D * 3 * D, 0.0), W2.b, 4 * D, 3 * D};
  for (int o = 0; o < D; ++o) a.W[(size_t)o * 3 * D + o] = 1.0;
  copy(Mat(a.W, D, 3 * D).block(0, D, D, 2 * D), W2.mat());
  a.W.insert(a.W.end(), low.W.begin(), low.W.end()); a.b.insert(a.b.end(), low.b.begin(), low.b.end());
  P.put_gemm("Wnext" + std::to_string(l), a);
}

// ---- entry points ---------------------------------------------------------------------------------------------------------------------

// the configurations the library takes, checked before anything else is looked at
inline int check_model_config(const LinetrModelConfig* cfg) {
  if (cfg->d_model != D || cfg->n_heads != HEADS) return fail(LINETR_E_ARG, "only descriptor_dim=256 / n_heads=4 are supported");
  if (cfg->d_inner % 128 != 0 || cfg->n_sig_layers < 0 || cfg->n_desc_layers < 1) return fail(LINETR_E_ARG, "bad d_inner / layer counts");
  const int e0 = cfg->enc_channels[0], e1 = cfg->enc_channels[1], e2 = cfg->enc_channels[2], e3 = cfg->enc_channels[3];
  if (e0 != 32 || e1 % 64 || e2 % 64 || e3 % 64 || e3 != D)
    return fail(LINETR_E_ARG, "keyline_encoder must be [32, 64k, 64k, 256] (got %d,%d,%d,%d)", e0, e1, e2, e3);
  return 0;
}

// The whole preparation of a configuration that passed check_model_config.  Placement order = order of the calls below.
inline int prepare_weights(const LinetrModelConfig& cfg, TensorMap& tm, Prepared& P) {
  const int* e = cfg.enc_channels;
  // the statistics scratch of linetr_forward_train is sized for BN_MAX_CHANNELS channels per BatchNorm layer
  if (cfg.bn_batch_stats && std::max(*std::max_element(e, e + 4), 2 * D) > BN_MAX_CHANNELS)
    return fail(LINETR_E_ARG, "create: a training-mode handle (bn_batch_stats = 1) takes keyline_encoder widths up to %d (got %d, %d, %d, %d)",
                BN_MAX_CHANNELS, e[0], e[1], e[2], e[3]);
  int bn_slot = 0;
  Affine W5word;
  if (int err = pos_encoders(cfg, tm, P, bn_slot, W5word)) return err;
  if (int err = descriptive_layer(cfg, tm, P, W5word)) return err;
  const int L = cfg.n_sig_layers;
  std::vector<Affine> qkv(L), W2(L);
  for (int l = 0; l < L; ++l)
    if (int err = signature_layer(cfg, tm, P, bn_slot, l, qkv[l], W2[l])) return err;
  for (int l = 0; l + 1 < L; ++l) wnext(P, l, W2[l], qkv[l + 1]);
  const Affine fin = tm.conv("final_proj", D, D);
  if (tm.err) return tm.err;
  P.put_gemm("Wfin", fin);
  // x_out = z + W2 hid + b2 behind the last signature layer and final_proj is linear (line_transformer.py:245), so
  //   final_proj(x_out) = [Wfin | Wfin W2] [z ; hid] + (Wfin b2 + bfin)
  if (L > 0) P.put_gemm("Wfin2", fold_inner(fin.mat(), fin.mat(), W2[L - 1], fin.b));
  return 0;
}

}  // namespace lt
