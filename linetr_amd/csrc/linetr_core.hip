// liblinetr_hip.so, translation unit 1 of 6: lifetime (the float64 weight preparation itself: lt_prepare.h), host pre-filter, the collective entry point
// and the profiling entry points of the C ABI declared in include/linetr_hip.h.  No device code lives here.
#include <dlfcn.h>

#include <algorithm>
#include <condition_variable>
#include <functional>
#include <numeric>
#include <thread>

#include "lt_handle.h"
#include "lt_prepare.h"

using namespace lt;

namespace {

// Persistent host worker pool (the batched pre-filter used to create and join 7 std::threads per call).
// Leaked on purpose: the workers are detached and live until process exit, so there is no static-destruction order
// problem when the library is unloaded from an interpreter that is shutting down.
class WorkPool {
 public:
  static WorkPool& get() {
    static WorkPool* p = new WorkPool();
    return *p;
  }
  int size() const { return n_workers_ + 1; }
  // runs fn(0..n-1), the calling thread takes part; one parallel region at a time
  void run(int n, const std::function<void(int)>& fn) {
    if (n <= 0) return;
    if (n == 1 || n_workers_ == 0) { for (int i = 0; i < n; ++i) fn(i); return; }
    std::lock_guard<std::mutex> region(region_);
    {
      std::lock_guard<std::mutex> lk(m_);
      job_ = &fn; n_jobs_ = n; next_ = 0; pending_ = n; ++gen_;
    }
    cv_work_.notify_all();
    drain();
    std::unique_lock<std::mutex> lk(m_);
    cv_done_.wait(lk, [&] { return pending_ == 0; });
    job_ = nullptr;
  }

 private:
  WorkPool() {
    // one process per GPU: the ranks of a node share its cores (LOCAL_WORLD_SIZE is set by torch.distributed.run);
    // LINETR_HOST_THREADS overrides (0 = run the pre-filter on the calling thread)
    unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    if (const char* lw = getenv("LOCAL_WORLD_SIZE")) hw /= (unsigned)std::max(1, atoi(lw));
    n_workers_ = (int)std::min(15u, hw > 1 ? hw / 2 : 0u);
    if (const char* ht = getenv("LINETR_HOST_THREADS")) n_workers_ = std::max(0, std::min(63, atoi(ht) - 1));
    for (int i = 0; i < n_workers_; ++i) std::thread([this] { loop(); }).detach();
  }
  void drain() {
    for (;;) {
      int i;
      const std::function<void(int)>* f;
      {
        std::lock_guard<std::mutex> lk(m_);
        if (!job_ || next_ >= n_jobs_) return;
        i = next_++;
        f = job_;
      }
      (*f)(i);
      std::lock_guard<std::mutex> lk(m_);
      if (--pending_ == 0) cv_done_.notify_all();
    }
  }
  void loop() {
    uint64_t seen = 0;
    for (;;) {
      {
        std::unique_lock<std::mutex> lk(m_);
        cv_work_.wait(lk, [&] { return gen_ != seen; });
        seen = gen_;
      }
      drain();
    }
  }
  std::mutex m_, region_;
  std::condition_variable cv_work_, cv_done_;
  const std::function<void(int)>* job_ = nullptr;
  int n_jobs_ = 0, next_ = 0, pending_ = 0, n_workers_ = 0;
  uint64_t gen_ = 0;
};

// Where the entries of the prepared table (lt_prepare.h) land in the handle, by entry name: GEMM weights (the bias goes along) and plain
// vectors.  The handle's per-layer vectors have their final size before this is called.
struct HandleSlots { std::map<std::string, GemmW*> gemm; std::map<std::string, const float**> vec; };
HandleSlots slots_of(LinetrHandle* H) {
  PosEncoder &w = H->enc[ENC_WORD], &l = H->enc[ENC_LINE];
  HandleSlots s{{{"Wword2", &w.W2}, {"Wword3", &w.W3}, {"Wword4", &w.W4}, {"Wline2", &l.W2}, {"Wline3", &l.W3}, {"Wline4", &l.W4},
                 {"Wline5", &H->lW5}, {"Watt", &H->Watt}, {"Wfc", &H->Wfc}, {"Wf1", &H->Wf1}, {"Wf2", &H->Wf2}, {"Wfin", &H->Wfin},
                 {"Wfin2", &H->Wfin2}},
                {{"Wword1", &w.W1}, {"bword1", &w.b1}, {"Wline1", &l.W1}, {"bline1", &l.b1}, {"U", &H->pool.U}, {"U2", &H->pool.U2},
                 {"ln1g", &H->ln1g}, {"ln1b", &H->ln1b}, {"ln2g", &H->ln2g}, {"ln2b", &H->ln2b}}};
  for (size_t i = 0; i < H->sig.size(); ++i) {
    const std::string n = std::to_string(i);
    s.gemm["Wqkv" + n] = &H->sig[i].Wqkv; s.gemm["W1m" + n] = &H->sig[i].W1; s.gemm["W2" + n] = &H->sig[i].W2; s.gemm["Wnext" + n] = &H->sig[i].Wnext;
  }
  for (size_t i = 0; i < H->bn_g.size(); ++i) { s.vec["bn_g" + std::to_string(i)] = &H->bn_g[i]; s.vec["bn_b" + std::to_string(i)] = &H->bn_b[i]; }
  return s;
}

// the state dict as an argument: a count and names a std::string can be made of (TensorMap, lt_prepare.h)
int check_tensor_table(int32_t n_tensors, const char* const* names) {
  if (n_tensors < 0) return fail(LINETR_E_ARG, "a negative number of state_dict tensors (%d)", n_tensors);
  for (int32_t i = 0; i < n_tensors; ++i)
    if (!names[i]) return fail(LINETR_E_ARG, "state_dict tensor %d has a NULL name", i);
  return 0;
}

}  // namespace

// =============================================================================================
// lifetime
// =============================================================================================

extern "C" int linetr_abi_version(void) { return LINETR_ABI_VERSION; }
extern "C" const char* linetr_last_error(void) { return g_err.c_str(); }

extern "C" int linetr_create(const LinetrModelConfig* cfg, int32_t n_tensors, const char* const* names,
                             const float* const* h_data, const int64_t* numel, int32_t device,
                             LinetrHandle** out) {
  if (!cfg || !out || !names || !h_data || !numel) return fail(LINETR_E_ARG, "null argument");
  if (int e = check_tensor_table(n_tensors, names)) return e;
  if (int e = check_model_config(cfg)) return e;
  int ndev = 0;
  LT_HIP(hipGetDeviceCount(&ndev));
  if (ndev <= 0 || device >= ndev) return fail(LINETR_E_HIP, "no usable HIP device (count=%d)", ndev);
  LT_HIP(hipSetDevice(device));

  // the weights, prepared in float64 on the host (lt_prepare.h), as one upload
  TensorMap tm(n_tensors, names, h_data, numel);
  Prepared P;
  if (int e = prepare_weights(*cfg, tm, P)) return e;
  auto H = std::make_unique<LinetrHandle>();
  H->cfg = *cfg; H->device = device;
  LT_HIP(hipMalloc((void**)&H->arena, P.image.size() * sizeof(float)));
  LT_HIP(hipMemcpy(H->arena, P.image.data(), P.image.size() * sizeof(float), hipMemcpyHostToDevice));
  // every table entry to its field.  A training-mode handle: gamma / beta / channel count of the 8 + n_sig_layers BatchNorm layers
  H->sig.resize(cfg->n_sig_layers);
  const size_t n_bn = cfg->bn_batch_stats ? 8 + cfg->n_sig_layers : 0;
  H->bn_g.resize(n_bn); H->bn_b.resize(n_bn); H->bn_c.resize(n_bn);
  const HandleSlots slots = slots_of(H.get());
  std::vector<GemmWSpec> gemm_w;
  for (size_t i = 0; i < P.table.size(); ++i) {
    const PreparedEntry& e = P.table[i];
    if (e.gemm) {   // a GEMM weight [rows, K] and, behind it, its bias
      GemmW* w = slots.gemm.at(e.name);
      w->W = H->arena + e.off; w->b = H->arena + P.table[++i].off; w->rows = e.rows; w->K = e.cols;
      gemm_w.push_back({w, e.st});
    } else {
      *slots.vec.at(e.name) = H->arena + e.off;
      if (e.name.compare(0, 4, "bn_g") == 0) H->bn_c[atoi(e.name.c_str() + 4)] = e.rows;   // bn_g<slot>: one row per channel
    }
  }
  for (int h = 0; h < HEADS; ++h) { H->pool.c_tok[h] = P.c_tok[h]; H->pool.s_cls[h] = P.s_cls[h]; }
  // split-precision copies of the GEMM weights: made on the device (linetr_net.hip owns the kernels)
  if (int e = make_split_copies(H.get(), gemm_w)) return e;
  if (const char* e = getenv("LINETR_PRECISION")) {
    if (!strcmp(e, "f32")) H->precision = LINETR_PREC_F32;
    else if (!strcmp(e, "bf16x3")) H->precision = LINETR_PREC_BF16X3;
    else if (!strcmp(e, "bf16x6")) H->precision = LINETR_PREC_BF16X6;
    else if (!strcmp(e, "f16x3")) H->precision = LINETR_PREC_F16X3;
    else return fail(LINETR_E_ARG, "LINETR_PRECISION must be f32, bf16x3, bf16x6 or f16x3 (got '%s')", e);
  }
  *out = H.release();
  return LINETR_OK;
}

extern "C" int linetr_debug_prepare(const LinetrModelConfig* cfg, int32_t n_tensors, const char* const* names, const float* const* h_data,
                                    const int64_t* numel, float* h_image, int64_t image_capacity, LinetrPreparedEntry* h_table,
                                    int32_t table_capacity, int64_t* n_floats, int32_t* n_entries) {
  if (!cfg || !names || !h_data || !numel || !n_floats || !n_entries) return fail(LINETR_E_ARG, "null argument");
  if (image_capacity < 0 || table_capacity < 0) return fail(LINETR_E_ARG, "debug_prepare: a negative capacity");
  if (int e = check_tensor_table(n_tensors, names)) return e;
  if (int e = check_model_config(cfg)) return e;
  TensorMap tm(n_tensors, names, h_data, numel);
  Prepared P;
  if (int e = prepare_weights(*cfg, tm, P)) return e;
  const size_t arena = P.image.size();
  *n_floats = (int64_t)arena + 2 * HEADS;
  *n_entries = (int32_t)P.table.size() + 2;
  if ((h_image && image_capacity < *n_floats) || (h_table && table_capacity < *n_entries))
    return fail(LINETR_E_CAPACITY, "debug_prepare: %lld floats and %d entries do not fit %lld and %d", (long long)*n_floats, *n_entries,
                (long long)image_capacity, table_capacity);
  if (h_image) {
    memcpy(h_image, P.image.data(), arena * sizeof(float));
    memcpy(h_image + arena, P.c_tok, HEADS * sizeof(float));
    memcpy(h_image + arena + HEADS, P.s_cls, HEADS * sizeof(float));
  }
  if (h_table) {
    P.table.push_back({"c_tok", arena, HEADS, 1, false, false});
    P.table.push_back({"s_cls", arena + HEADS, HEADS, 1, false, false});
    for (size_t i = 0; i < P.table.size(); ++i) {
      const PreparedEntry& e = P.table[i];
      LinetrPreparedEntry o{};
      snprintf(o.name, sizeof o.name, "%s", e.name.c_str());
      o.offset = (int64_t)e.off; o.rows = e.rows; o.cols = e.cols;
      o.flags = (e.gemm ? LINETR_PREP_GEMM : 0) | (e.st ? LINETR_PREP_ST : 0);
      h_table[i] = o;
    }
  }
  return LINETR_OK;
}

extern "C" int linetr_set_precision(LinetrHandle* h, int32_t mode) {
  if (!h || mode < LINETR_PREC_F32 || mode > LINETR_PREC_F16X3) return fail(LINETR_E_ARG, "bad precision mode");
  h->precision = mode;
  return LINETR_OK;
}
extern "C" int linetr_get_precision(const LinetrHandle* h) { return h ? h->precision : LINETR_E_ARG; }

extern "C" void linetr_destroy(LinetrHandle* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  for (auto& p : h->pending) { (void)hipEventDestroy(p.a); (void)hipEventDestroy(p.b); }
  for (auto e : h->event_pool) (void)hipEventDestroy(e);
  for (hipStream_t x : h->pipe.stream)
    if (x) { (void)hipStreamSynchronize(x); (void)hipStreamDestroy(x); }
  for (int s = 0; s < LinetrHandle::PIPE_SLOTS; ++s) {
    for (hipEvent_t e : {h->pipe.fork[s], h->pipe.done[s]})
      if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : h->pipe.cut[s])
      if (e) (void)hipEventDestroy(e);
  }
  if (h->arena) (void)hipFree(h->arena);
  if (h->split_arena) (void)hipFree(h->split_arena);
  if (h->zeros) (void)hipFree(h->zeros);
  if (h->w2p_arena) (void)hipFree(h->w2p_arena);
  if (h->sk_ws) (void)hipFree(h->sk_ws);
  if (h->sk_flags) (void)hipFree(h->sk_flags);
  if (h->pn_abort) (void)hipHostFree(h->pn_abort);
  for (auto& kv : h->debug_split) (void)hipFree(kv.second);
  delete h;
}

// =============================================================================================
// host pre-filter
// =============================================================================================

// what every packing entry point asks of its two tokeniser settings, lines or no lines (a NaN distance fails the comparison)
static int check_token_args(double td, int T) {
  if (!(td > 0) || T < 1) return fail(LINETR_E_ARG, "token_distance must be > 0 and max_tokens >= 1");
  return 0;
}

static int pack_one(LinetrLineRec& r, double td, int T, int image, int line_local, int& sub_cursor, int& tok_cursor) {
  if (int e = check_token_args(td, T)) return e;
  const double nt = std::ceil(r.length / td);          // line_process.py:109
  if (!(nt >= 1) || nt > 1e7) return fail(LINETR_E_ARG, "key-line %d has a non-positive / absurd token count", line_local);
  r.n_tok = (int)nt;
  r.n_sub = (r.n_tok + T - 1) / T;                      // :121
  r.first_sub = sub_cursor;
  r.image = image;
  r.line_local = line_local;
  r.first_tok = tok_cursor;
  if ((int64_t)sub_cursor + r.n_sub > INT32_MAX || (int64_t)tok_cursor + r.n_tok > INT32_MAX)
    return fail(LINETR_E_ARG, "more than 2^31 - 1 sub-lines or tokens in one batch (at key-line %d of image %d)", line_local, image);
  sub_cursor += r.n_sub;
  tok_cursor += r.n_tok;
  // the reference asserts every walked distance <= geometric length (:44-45)
  if (r.n_tok >= 2) {
    const double dx = r.ep[0] - r.sp[0], dy = r.ep[1] - r.sp[1];
    const double geo = std::sqrt(dx * dx + dy * dy);
    if (!(geo >= (double)(r.n_tok - 2) * td))
      return fail(LINETR_E_ASSERT, "distance should be smaller than line length! (key-line %d)", line_local);
  }
  return 0;
}

static void angle_of(LinetrLineRec& r) {  // line_process.py:28-41
  double th = std::atan2(r.ep[0] - r.sp[0], r.ep[1] - r.sp[1]);
  if (th < 0) th += M_PI;
#ifdef __GLIBC__
  // one libm call for both (glibc's sincos returns exactly what its sin and cos return)
  ::sincos(2 * th, &r.angle[1], &r.angle[0]);
#else
  r.angle[0] = std::cos(2 * th);
  r.angle[1] = std::sin(2 * th);
#endif
}

extern "C" int linetr_pack_lines(const double* h_klines, const double* h_length, const double* h_angles, int32_t K,
                                 double td, int32_t T, int32_t image_index, int32_t sub_base, int32_t tok_base,
                                 LinetrLineRec* h_recs, int32_t* n_out) {
  if (K < 0 || (K > 0 && (!h_klines || !h_length || !h_angles || !h_recs))) return fail(LINETR_E_ARG, "null argument");
  if (sub_base < 0 || tok_base < 0) return fail(LINETR_E_ARG, "pack_lines: a negative sub-line or token base");
  if (int e = check_token_args(td, T)) return e;
  int cur = sub_base, tcur = tok_base;
  for (int k = 0; k < K; ++k) {
    LinetrLineRec& r = h_recs[k];
    r.sp[0] = h_klines[k * 4 + 0]; r.sp[1] = h_klines[k * 4 + 1];
    r.ep[0] = h_klines[k * 4 + 2]; r.ep[1] = h_klines[k * 4 + 3];
    r.length = h_length[k];
    r.angle[0] = h_angles[k * 2]; r.angle[1] = h_angles[k * 2 + 1];
    if (int e = pack_one(r, td, T, image_index, k, cur, tcur)) return e;
  }
  if (n_out) *n_out = cur - sub_base;
  return LINETR_OK;
}

// ---- pseudo lines of the fixed-size training samples (dataloaders/utils/util_lines.py:559-668), float64 on the host ----------------

struct KeptLineAttr { double sp[2], ep[2], length; };
// one uniform double in [0, 1) from two Philox words: 53 bits, (hi >> 5) 2^26 + (lo >> 6) over 2^53
static double philox_u01(uint32_t hi, uint32_t lo) { return ((double)(hi >> 5) * 67108864.0 + (double)(lo >> 6)) / 9007199254740992.0; }

extern "C" int linetr_make_pseudo_lines(uint64_t seed, int32_t image_index, int32_t n, double shape0, double shape1, double min_length,
                                        double* h_lines) {
#pragma clang fp contract(off)
  constexpr double MASK = 15.0, MAX_RAND = 160.0;
  constexpr int MAX_ATTEMPTS = 64;
  if (n < 0 || (n > 0 && !h_lines) || image_index < 0 || seed >> 32) return fail(LINETR_E_ARG, "make_pseudo_lines: bad argument (a 32-bit seed, n >= 0)");
  if (!(min_length > 0) || !(min_length < MAX_RAND) || !(shape0 - MASK >= MASK + 2 * min_length) || !(shape1 - MASK >= MASK + 2 * min_length))
    return fail(LINETR_E_ARG, "make_pseudo_lines: image_shape (%g, %g) has no room for lines of min_length %g", shape0, shape1, min_length);
  const double area0 = shape0 - min_length - MASK, area1 = shape1 - min_length - MASK;     // util_lines.py:563
  for (int i = 0; i < n; ++i) {
    double* l = h_lines + (size_t)i * 4;
    int attempt = 0;
    for (; attempt < MAX_ATTEMPTS; ++attempt) {
      uint32_t a[4], b[4];
      philox4x32_10((uint32_t)i, (uint32_t)attempt, 0u, 0u, (uint32_t)seed, (uint32_t)image_index, a);
      philox4x32_10((uint32_t)i, (uint32_t)attempt, 1u, 0u, (uint32_t)seed, (uint32_t)image_index, b);
      const double sx = area0 * philox_u01(a[0], a[1]), sy = area1 * philox_u01(a[2], a[3]);        // :568
      const double ang = 2 * M_PI * philox_u01(b[0], b[1]);                                          // :571
      const double len = (MAX_RAND - min_length) * philox_u01(b[2], b[3]) + min_length;              // :573
      const double ex = sx + len * std::cos(ang), ey = sy + len * std::sin(ang);                     // :574-575
      l[0] = std::min(std::max(sx, MASK), shape0 - MASK);                                            // :576-577
      l[1] = std::min(std::max(sy, MASK), shape1 - MASK);
      l[2] = std::min(std::max(ex, MASK), shape0 - MASK);
      l[3] = std::min(std::max(ey, MASK), shape1 - MASK);
      const double dx = l[2] - l[0], dy = l[3] - l[1];
      const double length = std::sqrt(dx * dx + dy * dy);
      // the first draw stands unless it is shorter than min_length (:588); a redraw has to be longer (:610)
      if (attempt == 0 ? !(length < min_length) : length > min_length) break;
    }
    if (attempt == MAX_ATTEMPTS) {   // the reference would loop on: a fixed valid line instead
      l[0] = MASK; l[1] = MASK; l[2] = MASK + 2 * min_length; l[3] = MASK;
    }
  }
  return LINETR_OK;
}

extern "C" int linetr_find_line_attributes(const double* h_lines, int32_t n, double min_length, int32_t max_sublines, double* h_klines,
                                           double* h_length, double* h_angles, int32_t* n_out) {
#pragma clang fp contract(off)
  if (n < 0 || (n > 0 && (!h_lines || !h_klines || !h_length || !h_angles)) || !n_out) return fail(LINETR_E_ARG, "find_line_attributes: null argument");
  std::vector<KeptLineAttr> keep;
  keep.reserve(n);
  for (int i = 0; i < n; ++i) {
    const double* l = h_lines + (size_t)i * 4;
    // (a NaN length would pass the filter below and has no place in the sort's order)
    if (!std::isfinite(l[0]) || !std::isfinite(l[1]) || !std::isfinite(l[2]) || !std::isfinite(l[3]))
      return fail(LINETR_E_ARG, "find_line_attributes: line %d has a coordinate that is not finite", i);
    KeptLineAttr r;
    if (l[0] < l[2]) { r.sp[0] = l[0]; r.sp[1] = l[1]; r.ep[0] = l[2]; r.ep[1] = l[3]; }      // :641-646
    else { r.sp[0] = l[2]; r.sp[1] = l[3]; r.ep[0] = l[0]; r.ep[1] = l[1]; }
    const double dx = r.ep[0] - r.sp[0], dy = r.ep[1] - r.sp[1];
    r.length = std::sqrt(dx * dx + dy * dy);                                                    // :648
    if (r.length < min_length) continue;                                                        // :649
    keep.push_back(r);
  }
  // np.argsort, reversed (:662-663), under linetr_prefilter's tie rule: a stable ascending order read backwards
  std::vector<std::pair<double, int>> order(keep.size());
  for (size_t i = 0; i < keep.size(); ++i) order[i] = {keep[i].length, (int)i};
  std::stable_sort(order.begin(), order.end(), [](const std::pair<double, int>& a, const std::pair<double, int>& b) { return a.first < b.first; });
  int64_t n_keep = (int64_t)order.size();
  if (max_sublines < 0) n_keep = std::max<int64_t>(0, n_keep + max_sublines);                   // python slice [:m]
  else n_keep = std::min<int64_t>(n_keep, max_sublines);
  for (int64_t i = 0; i < n_keep; ++i) {
    const KeptLineAttr& kl = keep[order[order.size() - 1 - i].second];
    LinetrLineRec r{};
    r.sp[0] = kl.sp[0]; r.sp[1] = kl.sp[1]; r.ep[0] = kl.ep[0]; r.ep[1] = kl.ep[1];
    angle_of(r);                                                                                // get_angles, :619-632
    h_klines[i * 4 + 0] = kl.sp[0]; h_klines[i * 4 + 1] = kl.sp[1]; h_klines[i * 4 + 2] = kl.ep[0]; h_klines[i * 4 + 3] = kl.ep[1];
    h_length[i] = kl.length;
    h_angles[i * 2 + 0] = r.angle[0]; h_angles[i * 2 + 1] = r.angle[1];
  }
  *n_out = (int32_t)n_keep;
  return LINETR_OK;
}

// filter + sort of one image (records carry geometry/length/angle only).  `emit(n)` is called once with the number of surviving
// lines and returns where to write them: straight into the caller's record array on the single-thread path (a record is 80 bytes;
// the earlier form copied every survivor three times).
struct KeptLine { double sp[2], ep[2], length; };
// images of the last pre-filter call on this thread whose sorted candidates held equal lengths (linetr_prefilter_tied_images)
static thread_local std::vector<int32_t> g_tied_images;
template <class Emit>
static void prefilter_core(const double* L, int32_t K, int32_t height, int32_t width, int32_t border,
                           double min_length, int32_t max_keylines, const double* vm, bool* tied, Emit emit) {
  static thread_local std::vector<KeptLine> keep;
  static thread_local std::vector<std::pair<double, int>> order;
  keep.clear();
  keep.reserve(K);
  const double xmax = ((double)width - 0.001) - (double)border;   // width-eps-border, line_process.py:72-74
  const double ymax = ((double)height - 0.001) - (double)border;
  for (int k = 0; k < K; ++k) {
    const double* l = L + (size_t)k * 6;
    KeptLine r;
    if (l[0] < l[2]) { r.sp[0] = l[0]; r.sp[1] = l[1]; r.ep[0] = l[2]; r.ep[1] = l[3]; }   // :212-217
    else { r.sp[0] = l[2]; r.sp[1] = l[3]; r.ep[0] = l[0]; r.ep[1] = l[1]; }
    // lineLength * 2 ** octave (:220); an integral octave is an exact power of two either way: skip the pow call
    const double oct = l[5];
    r.length = (oct == std::floor(oct) && std::fabs(oct) < 64.0) ? l[4] * std::ldexp(1.0, (int)oct) : l[4] * std::pow(2.0, oct);
    const bool inside = r.sp[0] >= border && r.sp[0] < width - border && r.sp[1] >= border && r.sp[1] < height - border &&
                        r.ep[0] >= border && r.ep[0] < width - border && r.ep[1] >= border && r.ep[1] < height - border;
    if (!inside) continue;                                                                   // :62-70
    r.sp[0] = std::min(r.sp[0], xmax); r.ep[0] = std::min(r.ep[0], xmax);
    r.sp[1] = std::min(r.sp[1], ymax); r.ep[1] = std::min(r.ep[1], ymax);
    if (vm) {                                                                                // :76-80
      const int64_t sx = (int64_t)std::floor(r.sp[0]), sy = (int64_t)std::floor(r.sp[1]);
      const int64_t ex = (int64_t)std::floor(r.ep[0]), ey = (int64_t)std::floor(r.ep[1]);
      auto at = [&](int64_t y, int64_t x) {  // numpy-style wrap of negative indices
        if (y < 0) y += height;
        if (x < 0) x += width;
        return vm[y * width + x];
      };
      if (at(sy, sx) + at(ey, ex) == 0.0) continue;
    }
    if (!(r.length > min_length)) continue;                                                  // :8
    keep.push_back(r);
  }
  // ascending stable order by length, read backwards (:15-16): ties come out in descending input order, as before
  order.resize(keep.size());
  for (size_t i = 0; i < keep.size(); ++i) order[i] = {keep[i].length, (int)i};
  std::stable_sort(order.begin(), order.end(), [](const std::pair<double, int>& a, const std::pair<double, int>& b) { return a.first < b.first; });
  // equal lengths anywhere among the candidates (a tie across the [:max_keylines] cut changes the SET, not only the order)
  *tied = false;
  for (size_t i = 1; i < order.size(); ++i)
    if (order[i].first == order[i - 1].first) { *tied = true; break; }
  int64_t n_keep = (int64_t)order.size();
  if (max_keylines < 0) n_keep = std::max<int64_t>(0, n_keep + max_keylines);                // python slice [:m]
  else n_keep = std::min<int64_t>(n_keep, max_keylines);
  LinetrLineRec* out = emit(n_keep);
  if (!out) return;
  for (int64_t i = 0; i < n_keep; ++i) {
    const KeptLine& kl = keep[order[order.size() - 1 - i].second];
    LinetrLineRec r{};
    r.sp[0] = kl.sp[0]; r.sp[1] = kl.sp[1]; r.ep[0] = kl.ep[0]; r.ep[1] = kl.ep[1]; r.length = kl.length;
    angle_of(r);                                                                             // :20
    out[i] = r;
  }
}

// What both pre-filter entry points ask of the arguments they share, before a line is looked at.  A negative border would make the
// valid mask's index wrap a second time; a negative image size has no pixels to be inside of.
static int check_prefilter_args(int32_t height, int32_t width, int32_t border, double td, int32_t T, const LinetrLineRec* h_recs, int32_t capacity) {
  if (height < 0 || width < 0 || border < 0) return fail(LINETR_E_ARG, "prefilter: negative height, width or border (%d, %d, %d)", height, width, border);
  if (capacity < 0 || (capacity > 0 && !h_recs)) return fail(LINETR_E_ARG, "prefilter: a negative capacity, or records missing for a capacity of %d", capacity);
  return check_token_args(td, T);
}

extern "C" int linetr_prefilter(const double* L, int32_t K, int32_t height, int32_t width, int32_t border,
                                double min_length, int32_t max_keylines, const double* vm, double td, int32_t T,
                                int32_t image_index, int32_t sub_base, int32_t tok_base, LinetrLineRec* h_recs,
                                int32_t capacity, int32_t* k_out, int32_t* n_out) {
  if (K < 0 || (K > 0 && !L) || !k_out || !n_out) return fail(LINETR_E_ARG, "null argument");
  if (sub_base < 0 || tok_base < 0) return fail(LINETR_E_ARG, "prefilter: a negative sub-line or token base");
  if (int e = check_prefilter_args(height, width, border, td, T, h_recs, capacity)) return e;
  int64_t n_sel = -1;
  bool tied = false;
  g_tied_images.clear();
  prefilter_core(L, K, height, width, border, min_length, max_keylines, vm, &tied, [&](int64_t n) -> LinetrLineRec* {
    n_sel = n;
    return n <= capacity ? h_recs : nullptr;
  });
  if (tied) g_tied_images.push_back(0);
  if (n_sel > capacity) return fail(LINETR_E_CAPACITY, "prefilter: %lld lines exceed capacity %d", (long long)n_sel, capacity);
  int cur = sub_base, tcur = tok_base;
  for (int64_t i = 0; i < n_sel; ++i)
    if (int e = pack_one(h_recs[i], td, T, image_index, (int)i, cur, tcur)) return e;
  *k_out = (int)n_sel;
  *n_out = cur - sub_base;
  return LINETR_OK;
}

// The per-image body of both batched entry points, written once: image i is filtered with the settings image_of(i) returns
// (linetr_prefilter_batch: the same four scalars for every image; linetr_prefilter_ragged: the caller's table entry).  The callers
// have checked every argument that does not depend on the lines.
template <class ImageOf>
static int prefilter_images(const char* who, const double* L, const int32_t* off, int32_t B, ImageOf image_of, int32_t border,
                            int32_t max_keylines, int32_t T, int32_t n_threads, LinetrLineRec* h_recs, int32_t capacity,
                            int32_t* cu_k, int32_t* cu_n) {
  // the offset table: starts at or above 0 and never decreases (image i owns rows off[i] .. off[i + 1])
  if (off[0] < 0) return fail(LINETR_E_ARG, "%s: line offset 0 is negative (%d)", who, off[0]);
  for (int i = 0; i < B; ++i)
    if (off[i + 1] < off[i]) return fail(LINETR_E_ARG, "%s: line offset %d (%d) is below offset %d (%d)", who, i + 1, off[i + 1], i, off[i]);
  if (B > 0 && off[B] > off[0] && !L) return fail(LINETR_E_ARG, "null argument");
  WorkPool& pool = WorkPool::get();
  int nt = n_threads > 0 ? n_threads : pool.size();
  nt = std::max(1, std::min(nt, B / 4));  // not worth a hand-off for fewer than 4 images per chunk
  // contiguous chunks of images, a few per thread so that uneven images balance out
  const int chunks = nt == 1 ? 1 : std::min(B, nt * 2);
  cu_k[0] = cu_n[0] = 0;
  int cur = 0, tcur = 0;
  int64_t k = 0;
  g_tied_images.clear();
  if (chunks == 1) {
    // a single pair / a few images: no hand-off, and the survivors are written where they stay
    for (int i = 0; i < B; ++i) {
      int64_t n_sel = -1;
      bool tied = false;
      const LinetrPrefilterImage im = image_of(i);
      prefilter_core(L + (size_t)off[i] * 6, off[i + 1] - off[i], im.height, im.width, border, im.min_length, max_keylines,
                     im.valid_mask, &tied, [&](int64_t n) -> LinetrLineRec* {
                       n_sel = n;
                       return k + n <= capacity ? h_recs + k : nullptr;
                     });
      if (tied) g_tied_images.push_back(i);
      if (k + n_sel > capacity) return fail(LINETR_E_CAPACITY, "%s: more than %d surviving lines", who, capacity);
      for (int64_t j = 0; j < n_sel; ++j)
        if (int e = pack_one(h_recs[k + j], im.token_distance, T, i, (int)j, cur, tcur)) return e;
      k += n_sel;
      cu_k[i + 1] = (int)k;
      cu_n[i + 1] = cur;
    }
    return LINETR_OK;
  }
  std::vector<std::vector<LinetrLineRec>> sel(B);
  std::vector<char> tied_img(B, 0);
  auto work = [&](int c) {
    const int i0 = (int)((int64_t)B * c / chunks), i1 = (int)((int64_t)B * (c + 1) / chunks);
    for (int i = i0; i < i1; ++i) {
      bool tied = false;
      const LinetrPrefilterImage im = image_of(i);
      prefilter_core(L + (size_t)off[i] * 6, off[i + 1] - off[i], im.height, im.width, border, im.min_length, max_keylines,
                     im.valid_mask, &tied, [&](int64_t n) -> LinetrLineRec* {
                       sel[i].resize(n);
                       return sel[i].data();
                     });
      tied_img[i] = tied;
    }
  };
  pool.run(chunks, work);
  for (int i = 0; i < B; ++i)
    if (tied_img[i]) g_tied_images.push_back(i);
  for (int i = 0; i < B; ++i) {
    if (k + (int64_t)sel[i].size() > capacity)
      return fail(LINETR_E_CAPACITY, "%s: more than %d surviving lines", who, capacity);
    const double td = image_of(i).token_distance;
    for (size_t j = 0; j < sel[i].size(); ++j) {
      if (int e = pack_one(sel[i][j], td, T, i, (int)j, cur, tcur)) return e;
      h_recs[k++] = sel[i][j];
    }
    cu_k[i + 1] = (int)k;
    cu_n[i + 1] = cur;
  }
  return LINETR_OK;
}

extern "C" int linetr_prefilter_batch(const double* L, const int32_t* off, int32_t B, int32_t height, int32_t width,
                                      int32_t border, double min_length, int32_t max_keylines,
                                      const double* const* vms, double td, int32_t T, int32_t n_threads,
                                      LinetrLineRec* h_recs, int32_t capacity, int32_t* cu_k, int32_t* cu_n) {
  if (B < 0 || !off || !cu_k || !cu_n) return fail(LINETR_E_ARG, "null argument");
  if (n_threads < 0) return fail(LINETR_E_ARG, "prefilter_batch: n_threads %d (0 = the library's default)", n_threads);
  if (int e = check_prefilter_args(height, width, border, td, T, h_recs, capacity)) return e;
  // the ragged call with a constant table
  auto image_of = [&](int i) { return LinetrPrefilterImage{height, width, min_length, td, vms ? vms[i] : nullptr}; };
  return prefilter_images("prefilter_batch", L, off, B, image_of, border, max_keylines, T, n_threads, h_recs, capacity, cu_k, cu_n);
}

extern "C" int linetr_prefilter_ragged(const double* L, const int32_t* off, int32_t B, const LinetrPrefilterImage* h_images,
                                       int32_t border, int32_t max_keylines, int32_t T, int32_t n_threads, LinetrLineRec* h_recs,
                                       int32_t capacity, int32_t* cu_k, int32_t* cu_n) {
  if (B < 0 || !off || !cu_k || !cu_n || (B > 0 && !h_images)) return fail(LINETR_E_ARG, "null argument");
  if (n_threads < 0) return fail(LINETR_E_ARG, "prefilter_ragged: n_threads %d (0 = the library's default)", n_threads);
  // every image's settings, before a line is looked at (no image: what does not belong to one)
  if (int e = check_prefilter_args(0, 0, border, 1.0, T, h_recs, capacity)) return e;
  for (int i = 0; i < B; ++i)
    if (int e = check_prefilter_args(h_images[i].height, h_images[i].width, border, h_images[i].token_distance, T, h_recs, capacity)) return e;
  auto image_of = [&](int i) { return h_images[i]; };
  return prefilter_images("prefilter_ragged", L, off, B, image_of, border, max_keylines, T, n_threads, h_recs, capacity, cu_k, cu_n);
}

extern "C" int32_t linetr_prefilter_tied_images(int32_t* h_images, int32_t capacity) {
  const int32_t n = (int32_t)g_tied_images.size();
  for (int32_t i = 0; i < n && i < capacity && h_images; ++i) h_images[i] = g_tied_images[i];
  return n;
}

// =============================================================================================
// multi-GPU collective (C-ABI form of parallel.allgather_descriptors)
// =============================================================================================

// ncclResult_t ncclAllGather(const void* sendbuff, void* recvbuff, size_t sendcount, ncclDataType_t, ncclComm_t, hipStream_t)
typedef int (*allgather_fn)(const void*, void*, size_t, int, void*, hipStream_t);
static allgather_fn g_allgather = nullptr;
static std::mutex g_allgather_mu;

extern "C" int linetr_set_allgather_fn(void* fn) {
  std::lock_guard<std::mutex> lk(g_allgather_mu);
  g_allgather = reinterpret_cast<allgather_fn>(fn);
  return LINETR_OK;
}

extern "C" int linetr_allgather_desc(void* nccl_comm, const void* d_slab, void* d_out, int64_t slab_bytes, void* stream) {
  if (!nccl_comm || !d_slab || !d_out || slab_bytes <= 0) return fail(LINETR_E_ARG, "allgather_desc: bad argument");
  allgather_fn fn = nullptr;
  {
    std::lock_guard<std::mutex> lk(g_allgather_mu);
    fn = g_allgather;
    if (!fn) {   // not given by the caller: the first ncclAllGather the process-wide symbol resolution finds
      void* sym = dlsym(RTLD_DEFAULT, "ncclAllGather");
      for (const char* name : {"librccl.so", "librccl.so.1"}) {
        if (sym) break;
        if (void* lib = dlopen(name, RTLD_NOW | RTLD_NOLOAD)) sym = dlsym(lib, "ncclAllGather");   // only an ALREADY loaded RCCL
      }
      fn = g_allgather = reinterpret_cast<allgather_fn>(sym);
    }
  }
  if (!fn) return fail(LINETR_E_HIP, "allgather_desc: no RCCL (ncclAllGather) is loaded in this process");
  const int rc = fn(d_slab, d_out, (size_t)slab_bytes, /*ncclChar*/ 0, nccl_comm, (hipStream_t)stream);
  if (rc != 0) return fail(LINETR_E_HIP, "allgather_desc: ncclAllGather failed with ncclResult_t %d", rc);
  return LINETR_OK;
}

// =============================================================================================
// profiling
// =============================================================================================

extern "C" int linetr_set_profiling(LinetrHandle* h, int32_t on) {
  if (!h) return fail(LINETR_E_ARG, "null handle");
  for (auto& p : h->pending) { h->event_pool.push_back(p.a); h->event_pool.push_back(p.b); }
  h->pending.clear();
  h->classes.clear();
  h->profiling = on != 0;
  return LINETR_OK;
}

extern "C" int linetr_get_profile(LinetrHandle* h, LinetrProfileEntry* out, int32_t max_entries, int32_t* n_out) {
  if (!h || !n_out) return fail(LINETR_E_ARG, "null argument");
  LT_HIP(hipSetDevice(h->device));
  for (auto& p : h->pending) {
    LT_HIP(hipEventSynchronize(p.b));
    float ms = 0.f;
    LT_HIP(hipEventElapsedTime(&ms, p.a, p.b));
    h->classes[p.cls].ms += ms;
    h->event_pool.push_back(p.a);
    h->event_pool.push_back(p.b);
  }
  h->pending.clear();
  const int n = std::min<int>((int)h->classes.size(), max_entries);
  for (int i = 0; i < n; ++i) {
    out[i].name = h->classes[i].name;
    out[i].calls = h->classes[i].calls;
    out[i].ms = h->classes[i].ms;
    out[i].flops = h->classes[i].flops;
    out[i].bytes = h->classes[i].bytes;
  }
  *n_out = (int)h->classes.size();
  return LINETR_OK;
}
