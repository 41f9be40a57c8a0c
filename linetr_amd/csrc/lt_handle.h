// The library handle and what every translation unit of liblinetr_hip.so shares: the prepared-weight table, the per-kernel-class
// HIP-event profiler and the declarations of the few host functions that cross translation units.
//   linetr_core.hip   lifetime, host pre-filter, collective, profiling entry points.  linetr_create's float64 weight preparation is
//                     lt_prepare.h: host only, no handle, one function per fold; create uploads its image and binds the handle by table entry
//   linetr_net.hip    tokenise / forward / describe + the GEMM dispatcher and every model kernel (the experiments build includes
//                     experiments/csrc/lt_x_net.h into it: the host code of its alternative paths and the hooks that select them)
//   linetr_match.hip  matcher, dense-map producer, slab packing, SuperPoint's key-point branch
//   linetr_train.hip  training and evaluation: validation step, criterion gradient, backward of the 1x1 layers, the descriptor head and
//                     the neighbour-line attention, ground-truth line assignment, fixed-size samples (lt_fixedsize.h over lt_token.h,
//                     whose kernels are static: the header is compiled into this unit and into linetr_net.hip)
//   linetr_sp.hip     the image front end: the native SuperPoint encoder (its own LinetrSpEncoder object; no LinetrHandle state) and the
//                     homography views in front of it (lt_warp.h: warped image batches, valid masks, mask erosion)
//   linetr_det.hip    the line segment detector (lt_linedet.h): linetr_detect_lines and its two debug entry points; no LinetrHandle state
//   linetr_photo.hip  the photometric augmentation of the dataset builder (lt_photometric.h): host sampler, linetr_photometric,
//                     linetr_gaussian_blur; no LinetrHandle state
//   linetr_pair.hip   (experiments build only, experiments/csrc/) the single-pair persistent signature network
#pragma once
#include <algorithm>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "lt_common.h"

// One GEMM weight of the prepared arena, Y = A W^T + b with W [rows, K] row-major in fp32, and where its split-precision copies
// sit in split_arena (made once by make_split_copies; nullptr = none): the 2-plane bf16 split of the bf16x3 mode, the 3-plane
// one of bf16x6, the 2-plane fp16 split of f16x3, and the split-tile image (lt_st_image.h) of the kernels that stream it.
struct GemmW {
  const float* W = nullptr;
  const float* b = nullptr;
  int rows = 0, K = 0;
  const unsigned char *s2 = nullptr, *s3 = nullptr, *h2 = nullptr, *st = nullptr;
};

struct SigLayer {
  GemmW Wqkv, W1, W2;   // merge conv folded into W1
  GemmW W2p;            // experiments build: W2 with K permuted inside 16-groups (lt_mlp_fused.h)
  // [x_out | q/k/v of the NEXT layer] = Wnext [z ; hid] + bnext: W2 + residual and the next projection as ONE contraction
  // ([4D x 3D]; all layers but the last).  Used for single-pair sizes only, where a dependent launch costs more than its flops.
  GemmW Wnext;
};

// layers 1-4 of a positional encoder: conv + BN + ReLU each; the first layer (3 or 5 inputs) is no GEMM
struct PosEncoder {
  const float *W1 = nullptr, *b1 = nullptr;
  GemmW W2, W3, W4;
};
enum { ENC_WORD = 0, ENC_LINE = 1 };

struct ProfClass {
  const char* name;
  int calls = 0;
  double flops = 0, bytes = 0;
  float ms = 0;
};

struct LinetrHandle {
  LinetrModelConfig cfg;
  int device = 0;
  float* arena = nullptr;  // all prepared weights, one allocation
  // the positional encoders (BN folded), ENC_WORD and ENC_LINE.  The line encoder's last (linear) layer is lW5; the word encoder's
  // is applied after pooling and lives in pool.U2
  PosEncoder enc[2];
  GemmW lW5;
  // line-descriptive layer (CLS-row algebra)
  lt::ClsPoolConst pool;
  GemmW Watt, Wfc, Wf1, Wf2;
  const float *ln1g, *ln1b, *ln2g, *ln2b;
  std::vector<SigLayer> sig;
  // training-mode handle (cfg.bn_batch_stats): gamma / beta / channel count of every BatchNorm layer, in the order of the packed
  // statistics arrays of linetr_forward_train (word encoder x4, line encoder x4, one per signature layer)
  std::vector<const float*> bn_g, bn_b;
  std::vector<int> bn_c;
  GemmW Wfin;
  GemmW Wfin2;   // final projection with the last signature layer's second MLP GEMM folded in (no signature layers: none)
  int precision = LINETR_PREC_BF16X6;
  unsigned char* split_arena = nullptr;   // the split copies of every GemmW above, one allocation
  std::map<const float*, unsigned char*> debug_split;  // linetr_debug_gemm(cache_weights=1): its split copies, by fp32 pointer
  // software pipeline of CONSECUTIVE describe calls (linetr_describe_submit / linetr_describe_join): a batch is cut into stages at
  // fixed points of the network (PipePlan), stage k of every batch runs on stream k, so stage k of batch i + 1 overlaps stage k + 1 of
  // batch i -- HBM-bound kernels under MFMA-bound ones, and the CUs a GEMM's last tile round leaves empty under another launch.
  // A batch in flight owns slot i mod LT_PIPE_SLOTS (its workspace + events).
  static constexpr int PIPE_SLOTS = 4, PIPE_STREAMS = 4;
  struct Pipe {
    hipStream_t stream[PIPE_STREAMS] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t fork[PIPE_SLOTS] = {}, done[PIPE_SLOTS] = {}, cut[PIPE_SLOTS][PIPE_STREAMS - 1] = {};
    bool submitted[PIPE_SLOTS] = {false, false, false, false};
    bool failed = false;
  } pipe;
  float* zeros = nullptr;   // 4096 zero floats: the "no bias" vector of the split-tile GEMM (experiments/csrc/lt_gemm_st.h)
  float* w2p_arena = nullptr;   // experiments build: every SigLayer::W2p, one allocation (experiments/csrc/lt_x_net.h)
  // stream-K workspace of the 128x256 GEMM (partial accumulator tiles + flags, one slot per CU; experiments/csrc/lt_gemm_sk.h)
  float* sk_ws = nullptr;
  unsigned* sk_flags = nullptr;
  unsigned sk_epoch = 0;
  // single-pair persistent signature network (lt_pairnet.h, linetr_pair.hip)
  unsigned* pn_abort = nullptr;       // host-mapped word a timed-out launch raises (read by the host before the next launch)
  unsigned* pn_abort_dev = nullptr;   // the same word as the device sees it
  bool pn_disabled = false;
  unsigned long long* pn_stamps = nullptr;   // diagnostics buffer (experiments build: linetr_debug_pairnet_stamps)
  int n_cu = 0;
  // profiling
  bool profiling = false;
  std::vector<ProfClass> classes;
  struct Pending { int cls; hipEvent_t a, b; };
  std::vector<Pending> pending;
  std::vector<hipEvent_t> event_pool;
};

namespace lt {

inline int prof_class(LinetrHandle* h, const char* name) {
  for (size_t i = 0; i < h->classes.size(); ++i)
    if (h->classes[i].name == name || strcmp(h->classes[i].name, name) == 0) return (int)i;
  ProfClass c;
  c.name = name;
  h->classes.push_back(c);
  return (int)h->classes.size() - 1;
}

inline hipEvent_t prof_event(LinetrHandle* h) {
  if (!h->event_pool.empty()) {
    hipEvent_t e = h->event_pool.back();
    h->event_pool.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  (void)hipEventCreate(&e);   // a null event only loses this kernel's timing sample
  return e;
}

// RAII bracket around one kernel launch
struct ProfScope {
  LinetrHandle* h;
  hipStream_t st;
  int cls = -1;
  hipEvent_t a{}, b{};
  ProfScope(LinetrHandle* h_, hipStream_t st_, const char* name, double flops, double bytes) : h(h_), st(st_) {
    if (!h || !h->profiling) return;
    cls = prof_class(h, name);
    h->classes[cls].calls++;
    h->classes[cls].flops += flops;
    h->classes[cls].bytes += bytes;
    a = prof_event(h);
    b = prof_event(h);
    (void)hipEventRecord(a, st);
  }
  ~ProfScope() {
    if (cls < 0) return;
    (void)hipEventRecord(b, st);
    h->pending.push_back({cls, a, b});
  }
};

// Pinned staging ring for the small host tables an entry point uploads (the matcher's PairDesc array and identity maps, the image
// table of linetr_describe_ragged).  A slot is
// reused only after the copy that read it has completed (event), so no entry point has to synchronise the stream.
struct PinnedRing {
  struct Slot { void* p = nullptr; size_t cap = 0; hipEvent_t ev = nullptr; bool busy = false; };
  Slot slots[8];
  int next = 0;
  std::mutex m;
  // returns a host pointer of >= bytes, or nullptr; *slot_out identifies the slot for commit()
  void* acquire(size_t bytes, int* slot_out) {
    std::lock_guard<std::mutex> lk(m);
    Slot& s = slots[next];
    *slot_out = next;
    next = (next + 1) % 8;
    if (s.busy) { (void)hipEventSynchronize(s.ev); s.busy = false; }
    if (s.cap < bytes) {
      if (s.p) (void)hipHostFree(s.p);
      s.p = nullptr; s.cap = 0;
      const size_t cap = std::max<size_t>(align_up((int64_t)bytes * 2, 4096), 16384);
      if (hipHostMalloc(&s.p, cap, hipHostMallocDefault) != hipSuccess) { s.p = nullptr; return nullptr; }
      s.cap = cap;
    }
    if (!s.ev && hipEventCreateWithFlags(&s.ev, hipEventDisableTiming) != hipSuccess) { s.ev = nullptr; return nullptr; }
    return s.p;
  }
  int commit(int slot, hipStream_t st) {   // call after the last async copy out of the slot has been enqueued
    std::lock_guard<std::mutex> lk(m);
    LT_HIP(hipEventRecord(slots[slot].ev, st));
    slots[slot].busy = true;
    return 0;
  }
};
inline PinnedRing& staging_ring() {   // one ring per device (its events belong to the device current at creation); leaked: see WorkPool
  static PinnedRing* rings[64] = {};
  static std::mutex m;
  int dev = 0;
  (void)hipGetDevice(&dev);
  std::lock_guard<std::mutex> lk(m);
  PinnedRing*& r = rings[dev & 63];
  if (!r) r = new PinnedRing();
  return *r;
}

// one GEMM weight of the prepared arena that needs split-precision copies (made on the device by linetr_net.hip, which points the
// GemmW at them); st: a split-tile image as well
struct GemmWSpec { GemmW* w; bool st; };
int make_split_copies(LinetrHandle* H, std::vector<GemmWSpec> weights);

}  // namespace lt
