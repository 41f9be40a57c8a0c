// liblinetr_hip.so, translation unit 3 of 4: the descriptor-distance matcher, the dense-map producer and the slab packing of the
// multi-GPU path (C ABI in include/linetr_hip.h; kernels in lt_match.h, lt_producer.h), SuperPoint's key-point branch (lt_keypoints.h), the
// validation step (lt_valstep.h), the criterion's gradient (lt_lossgrad.h), the backward of the 1x1 layers and the descriptor head
// (lt_linbwd.h), the neighbour-line attention's forward with statistics and backward (lt_attnbwd.h) and the ground-truth line assignment
// in front of them (lt_gtassign.h).
#include <algorithm>
#include <numeric>

#include "lt_handle.h"
#include "lt_match.h"
#include "lt_valstep.h"
#include "lt_lossgrad.h"
#include "lt_linbwd.h"
#include "lt_attnbwd.h"
#include "lt_gtassign.h"
#include "lt_producer.h"
#include "lt_keypoints.h"

using namespace lt;

// =============================================================================================
// matcher
// =============================================================================================

namespace {
// Pinned staging ring for the small host tables the matcher uploads (PairDesc array, identity maps).  A slot is
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
PinnedRing& staging_ring() {   // one ring per device (its events belong to the device current at creation); leaked: see WorkPool
  static PinnedRing* rings[64] = {};
  static std::mutex m;
  int dev = 0;
  (void)hipGetDevice(&dev);
  std::lock_guard<std::mutex> lk(m);
  PinnedRing*& r = rings[dev & 63];
  if (!r) r = new PinnedRing();
  return *r;
}

// Scratch of the one-launch single-pair matcher (pair_match_fused_kernel): column keys, row results, arrival counter.  One slot per
// (device, stream): launches on a stream are ordered and the kernel leaves its slot clean, so a slot is never shared by two
// launches in flight.  A slot is initialised (column and row keys all-ones, counter 0) by memsets queued on ITS stream in front of
// its first launch -- nothing is synchronised.  At most PAIR_SLOTS_MAX slots are kept (they are never freed: a stream handle may still
// have work in flight); a caller beyond that, or one whose allocation fails, gets nullptr and takes the three launches.
constexpr size_t PAIR_SLOTS_MAX = 256;
PairSlot* pair_slot(hipStream_t st) {
  static std::mutex m;
  static std::map<std::pair<int, hipStream_t>, PairSlot> slots;
  int dev = 0;
  (void)hipGetDevice(&dev);
  std::lock_guard<std::mutex> lk(m);
  auto it = slots.find({dev, st});
  if (it != slots.end()) return &it->second;
  if (slots.size() >= PAIR_SLOTS_MAX) return nullptr;
  char* mem = nullptr;
  const size_t bytes = (size_t)PF_MAX_K * 16 + 256;
  if (hipMalloc((void**)&mem, bytes) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
  if (hipMemsetAsync(mem, 0xff, (size_t)PF_MAX_K * 16, st) != hipSuccess ||
      hipMemsetAsync(mem + (size_t)PF_MAX_K * 16, 0, 256, st) != hipSuccess) {
    (void)hipGetLastError();
    (void)hipFree(mem);
    return nullptr;
  }
  PairSlot ps;
  ps.col_best = (unsigned long long*)mem;
  ps.row_res = (unsigned long long*)(mem + (size_t)PF_MAX_K * 8);
  ps.counter = (unsigned*)(mem + (size_t)PF_MAX_K * 16);
  return &(slots[{dev, st}] = ps);
}

// the one-launch matcher needs up to pair_fused_lds(PF_MAX_N1, PF_MAX_N1) bytes of dynamic LDS; a device that refuses keeps the
// three launches
bool fused_pair_lds_ok() {
  const int want = (int)pair_fused_lds(PF_MAX_N1, PF_MAX_N1);
  return allow_dynamic_lds<pair_match_fused_kernel<false>>(want) == hipSuccess &&
         allow_dynamic_lds<pair_match_fused_kernel<true>>(want) == hipSuccess;
}

// does a single-pair call have the sizes of the one-launch matcher (pair_match_fused_kernel)?
bool fused_pair_applies(int n0, int k0, int n1, int k1) {
  (void)n0;
  return k0 > 0 && k1 > 0 && n1 <= PF_MAX_N1 && k0 <= PF_MAX_K && k1 <= PF_MAX_K;
}

// the scratch slot of a single-pair call that takes the one-launch matcher, or nullptr (sizes beyond it, no LDS, no slot): then the
// three launches run.  Idempotent per (device, stream): linetr_match_points asks first (it skips the identity maps the one-launch
// path never reads) and linetr_match_gathered gets the same answer.
PairSlot* fused_pair_slot(int n0, int k0, int n1, int k1, hipStream_t st) {
  return fused_pair_applies(n0, k0, n1, k1) && fused_pair_lds_ok() ? pair_slot(st) : nullptr;
}

// ints of argmin scratch one pair needs (layout in lt_match.h)
int64_t pair_scratch_ints(int k0, int k1) { return 2 * (int64_t)k0 + 2 * (int64_t)k1 + 1 + 2 * (int64_t)cdiv(std::max(k0, 1), PM_ROWS) * k1 + 8; }
}  // namespace

extern "C" int64_t linetr_match_workspace_bytes(int32_t n_pairs, int64_t sum_n0n1, int64_t sum_k0k1, int64_t sum_k) {
  (void)sum_k0k1;
  // scratch bound: sum over pairs of pair_scratch_ints(k0,k1) <= 4 sum_k + 2 (sum_k0k1 / PM_ROWS + sum_k) + 9 P, and
  // k0 k1 <= n0 n1
  const int64_t scratch = 6 * sum_k + 2 * (sum_n0n1 / PM_ROWS + 1) + 9 * (int64_t)n_pairs;
  return align_up((int64_t)n_pairs * sizeof(PairDesc), 256) + align_up(sum_n0n1 * 4, 256) + align_up(scratch * 4, 256) + 256;
}

namespace {
// What linetr_debug_match forces (-1 everywhere: nothing, the product's own choices).  path: 0 the three launches, 1 / 2
// pair_match_fused_kernel<false> / <true>; seg1_global, cache_dk, device_table (read on the three-launch path): 0 / 1.
struct MatchForce { int path = -1, seg1_global = -1, cache_dk = -1, device_table = -1; };
int match_run(LinetrHandle* h, int32_t P, const int32_t* dims, const float* d_desc0, const int64_t* off_n0, const int32_t* d_s2l0,
              const int64_t* off_s0, const float* d_desc1, const int64_t* off_n1, const int32_t* d_s2l1, const int64_t* off_s1,
              float thr, int32_t mutual, float* d_dk, const int64_t* off_dk, int32_t* d_match01, const int64_t* off_k0, void* d_ws,
              int64_t ws_bytes, void* stream, const MatchForce& force, int32_t* path_used);
}  // namespace

extern "C" int linetr_match(LinetrHandle* h, int32_t P, const int32_t* dims, const float* d_desc0, const int64_t* off_n0,
                            const int32_t* d_s2l0, const float* d_desc1, const int64_t* off_n1, const int32_t* d_s2l1,
                            float thr, int32_t mutual, float* d_dk, const int64_t* off_dk, int32_t* d_match01,
                            const int64_t* off_k0, void* d_ws, int64_t ws_bytes, void* stream) {
  return match_run(h, P, dims, d_desc0, off_n0, d_s2l0, nullptr, d_desc1, off_n1, d_s2l1, nullptr, thr, mutual, d_dk, off_dk,
                   d_match01, off_k0, d_ws, ws_bytes, stream, MatchForce{}, nullptr);
}

extern "C" int linetr_match_gathered(LinetrHandle* h, int32_t P, const int32_t* dims, const float* d_desc0,
                                     const int64_t* off_n0, const int32_t* d_s2l0, const int64_t* off_s0,
                                     const float* d_desc1, const int64_t* off_n1, const int32_t* d_s2l1,
                                     const int64_t* off_s1, float thr, int32_t mutual, float* d_dk, const int64_t* off_dk,
                                     int32_t* d_match01, const int64_t* off_k0, void* d_ws, int64_t ws_bytes, void* stream) {
  return match_run(h, P, dims, d_desc0, off_n0, d_s2l0, off_s0, d_desc1, off_n1, d_s2l1, off_s1, thr, mutual, d_dk, off_dk,
                   d_match01, off_k0, d_ws, ws_bytes, stream, MatchForce{}, nullptr);
}

namespace {
// The matcher's paths (the numbers are linetr_debug_match's `path` argument, include/linetr_hip.h)
enum { MATCH_THREE = 0, MATCH_FUSED = 1, MATCH_FUSED_IDENT = 2 };

// The ONE body of the matcher: linetr_match / linetr_match_gathered pass "nothing forced", linetr_debug_match what its caller asks for
// (already checked there: a forced path never arrives here with sizes it does not serve).
int match_run(LinetrHandle* h, int32_t P, const int32_t* dims, const float* d_desc0, const int64_t* off_n0, const int32_t* d_s2l0,
              const int64_t* off_s0, const float* d_desc1, const int64_t* off_n1, const int32_t* d_s2l1, const int64_t* off_s1,
              float thr, int32_t mutual, float* d_dk, const int64_t* off_dk, int32_t* d_match01, const int64_t* off_k0, void* d_ws,
              int64_t ws_bytes, void* stream, const MatchForce& force, int32_t* path_used) {
  if (P < 0) return fail(LINETR_E_ARG, "match: bad argument");
  if (P == 0) return LINETR_OK;
  if (!dims || !off_n0 || !off_n1 || !off_dk || !off_k0 || !d_ws) return fail(LINETR_E_ARG, "match: null argument");
  hipStream_t st = (hipStream_t)stream;
  if (h) LT_HIP(hipSetDevice(h->device));
  PairTable tab{};
  int slot = -1;
  PairDesc* pd = tab.inl;
  const bool device_table = force.device_table < 0 ? P > PT_INLINE : force.device_table != 0;
  if (device_table) {
    pd = (PairDesc*)staging_ring().acquire((size_t)P * sizeof(PairDesc), &slot);
    if (!pd) return fail(LINETR_E_HIP, "match: pinned staging allocation failed");
  } else {
    tab.n_inline = P;
  }
  int64_t od = 0, os = 0, sum_k = 0;
  int max_n0 = 0, max_n1 = 0, max_k1 = 0, max_chunks = 0;
  double flops = 0;
  for (int p = 0; p < P; ++p) {
    PairDesc& d = pd[p];
    d.n0 = dims[p * 4 + 0]; d.k0 = dims[p * 4 + 1]; d.n1 = dims[p * 4 + 2]; d.k1 = dims[p * 4 + 3];
    if (d.n0 < 0 || d.n1 < 0 || d.k0 < 0 || d.k1 < 0 || d.k0 > d.n0 || d.k1 > d.n1)
      return fail(LINETR_E_ARG, "match: bad dims for pair %d", p);
    d.off_n0 = off_n0[p]; d.off_n1 = off_n1[p]; d.off_dk = off_dk[p]; d.off_k0 = off_k0[p];
    d.off_s0 = off_s0 ? off_s0[p] : off_n0[p];
    d.off_s1 = off_s1 ? off_s1[p] : off_n1[p];
    d.off_d = od; od += (int64_t)d.n0 * d.n1;
    d.chunks = cdiv(std::max(d.k0, 1), PM_ROWS);
    d.pad_ = 0;
    d.off_seg = os; os += pair_scratch_ints(d.k0, d.k1);
    sum_k += d.k0 + d.k1;
    max_n0 = std::max(max_n0, d.n0); max_n1 = std::max(max_n1, d.n1);
    max_k1 = std::max(max_k1, d.k1); max_chunks = std::max(max_chunks, d.chunks);
    flops += 2.0 * d.n0 * d.n1 * D;
  }
  if (ws_bytes < linetr_match_workspace_bytes(P, od, 0, sum_k)) return fail(LINETR_E_WORKSPACE, "match: workspace too small");
  char* base = (char*)d_ws;
  PairDesc* d_pd = (PairDesc*)base;
  float* d_dist = (float*)(base + align_up((int64_t)P * sizeof(PairDesc), 256));
  int* d_scr = (int*)((char*)d_dist + align_up(od * 4, 256));
  if (slot >= 0) {
    LT_HIP(hipMemcpyAsync(d_pd, pd, P * sizeof(PairDesc), hipMemcpyHostToDevice, st));
    if (int e = staging_ring().commit(slot, st)) return e;
    tab.ptr = d_pd;
  }
  if (max_n0 > 0 && max_n1 > 0) {
    if (!d_desc0 || !d_desc1 || !d_s2l0 || !d_s2l1 || !d_dk) return fail(LINETR_E_ARG, "match: null tensor");
    // A single pair of ordinary size: ONE launch (pair_match_fused_kernel, lt_match.h).  (r03 built a one-launch form that staged
    // 8 K steps through LDS with a load round trip exposed at each and lost to the three launches, 0.10 vs 0.08 ms; this one keeps
    // whole operand rows in registers -- two exposed round trips in all -- and combines the column argmin with one 64-bit atomicMin.)
    PairSlot* ps_ = P == 1 && force.path != MATCH_THREE ? fused_pair_slot(pd[0].n0, pd[0].k0, pd[0].n1, pd[0].k1, st) : nullptr;
    if (!ps_ && force.path > MATCH_THREE)      // a forced one-launch path never becomes the three launches
      return fused_pair_lds_ok() ? fail(LINETR_E_HIP, "match: no scratch slot for the one-launch matcher on this stream")
                                 : fail(LINETR_E_HIP, "match: the device refuses the one-launch matcher's dynamic LDS");
    if (ps_) {    // (no slot / no LDS: the three launches below)
      const PairDesc& d = pd[0];
      const size_t lds = pair_fused_lds(d.n1, d.k1);
      ProfScope ps(h, st, "pair_match_fused", flops, 4.0 * ((double)(d.n0 + d.n1) * D + (double)d.k0 * d.k1));
      // one sub-line per key-line on both sides (known from the counts alone: the maps are onto): Dk = D, columns split over two
      // blocks when a wave would otherwise multiply two tiles
      const bool ident = force.path < 0 ? d.n0 == d.k0 && d.n1 == d.k1 : force.path == MATCH_FUSED_IDENT;
      if (path_used) *path_used = ident ? MATCH_FUSED_IDENT : MATCH_FUSED;
      const float* a0 = d_desc0 + d.off_n0 * D; const float* a1 = d_desc1 + d.off_n1 * D;
      if (ident) {
        const int n_ct = cdiv(d.n1, 16);
        hipLaunchKernelGGL(pair_match_fused_kernel<true>, dim3(cdiv(d.k0, PM_ROWS), cdiv(n_ct, 8)), dim3(512), lds, st, a0, a1,
                           d_s2l0 + d.off_s0, d_s2l1 + d.off_s1, d.n0, d.k0, d.n1, d.k1, thr, mutual, d_dk + d.off_dk,
                           d_match01 + d.off_k0, *ps_);
      } else {
        hipLaunchKernelGGL(pair_match_fused_kernel<false>, dim3(cdiv(d.k0, PM_ROWS)), dim3(512), lds, st, a0, a1, d_s2l0 + d.off_s0,
                           d_s2l1 + d.off_s1, d.n0, d.k0, d.n1, d.k1, thr, mutual, d_dk + d.off_dk, d_match01 + d.off_k0, *ps_);
      }
      LT_LAUNCH_CHECK();
      return LINETR_OK;
    }
    ProfScope ps(h, st, "pair_dist", flops, 0);
    hipLaunchKernelGGL(pair_dist_kernel, dim3(cdiv(max_n1, 64), cdiv(max_n0, 64), P), dim3(256), 0, st, tab, d_desc0,
                       d_desc1, d_dist);
    LT_LAUNCH_CHECK();
  }
  {
    ProfScope ps(h, st, "pair_match", 0, 0);
    if (max_k1 > 0) {
      const int seg1_global = force.seg1_global < 0 ? max_k1 > PM_MAX_K1 : force.seg1_global;    // the reference has no limit (max_keylines / max_keypoints = -1)
      if (seg1_global) {
        hipLaunchKernelGGL(pair_seg1_kernel, dim3(cdiv(max_n1, 2048), P), dim3(256), 0, st, tab, d_s2l1, d_scr);
        LT_LAUNCH_CHECK();
      }
      const int cache_dk = force.cache_dk < 0 ? max_k1 <= PM_CACHE_K1 : force.cache_dk;
      hipLaunchKernelGGL(pair_pool_kernel, dim3(max_chunks, P), dim3(256), pair_pool_lds(max_k1, seg1_global, cache_dk), st, tab, d_s2l0,
                         d_s2l1, d_dist, d_dk, d_scr, seg1_global, cache_dk);
      LT_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(pair_final_kernel, dim3(P), dim3(256), 0, st, tab, thr, mutual, d_match01, d_scr);
    LT_LAUNCH_CHECK();
  }
  if (path_used) *path_used = MATCH_THREE;
  return LINETR_OK;   // fully asynchronous: the pair table travels in the kernel arguments or in ring-owned pinned memory
}
}  // namespace

extern "C" int linetr_debug_match(LinetrHandle* h, int32_t P, const int32_t* dims, const float* d_desc0, const int64_t* off_n0,
                                  const int32_t* d_s2l0, const float* d_desc1, const int64_t* off_n1, const int32_t* d_s2l1, float thr,
                                  int32_t mutual, float* d_dk, const int64_t* off_dk, int32_t* d_match01, const int64_t* off_k0,
                                  void* d_ws, int64_t ws_bytes, int32_t path, int32_t seg1_global, int32_t cache_dk,
                                  int32_t device_table, int32_t* path_used, void* stream) {
  if (P < 1 || !dims) return fail(LINETR_E_ARG, "debug_match: at least one pair and its dims expected");
  if (path < -1 || path > MATCH_FUSED_IDENT) return fail(LINETR_E_ARG, "debug_match: path must be -1 .. 2");
  for (const int v : {seg1_global, cache_dk, device_table})
    if (v < -1 || v > 1) return fail(LINETR_E_ARG, "debug_match: seg1_global, cache_dk and device_table must be -1, 0 or 1");
  if (path != MATCH_THREE && (seg1_global >= 0 || cache_dk >= 0 || device_table >= 0))
    return fail(LINETR_E_ARG, "debug_match: seg1_global, cache_dk and device_table are forced on path 0 only");
  int max_k1 = 0;
  for (int p = 0; p < P; ++p) {
    const int32_t* d = dims + 4 * p;
    if (d[0] < 0 || d[1] < 0 || d[2] < 0 || d[3] < 0 || d[1] > d[0] || d[3] > d[2]) return fail(LINETR_E_ARG, "debug_match: bad dims for pair %d", p);
    max_k1 = std::max(max_k1, d[3]);
  }
  if (path > MATCH_THREE) {
    if (P != 1) return fail(LINETR_E_ARG, "debug_match: the one-launch matcher takes one pair, not %d", P);
    if (!fused_pair_applies(dims[0], dims[1], dims[2], dims[3]))
      return fail(LINETR_E_ARG, "debug_match: sizes beyond the one-launch matcher (k0, k1 in 1 .. %d, n1 <= %d)", PF_MAX_K, PF_MAX_N1);
    if (path == MATCH_FUSED_IDENT && (dims[0] != dims[1] || dims[2] != dims[3]))
      return fail(LINETR_E_ARG, "debug_match: the identity kernel needs one sub-line per key-line on both sides");
  }
  if (cache_dk == 1 && max_k1 > PM_CACHE_K1) return fail(LINETR_E_ARG, "debug_match: %d pooled columns do not fit the LDS row cache (%d)", max_k1, PM_CACHE_K1);
  if (seg1_global == 0 && max_k1 > PM_MAX_K1) return fail(LINETR_E_ARG, "debug_match: a segment table of %d key-lines does not fit the LDS (%d)", max_k1, PM_MAX_K1);
  if (device_table == 0 && P > PT_INLINE) return fail(LINETR_E_ARG, "debug_match: %d pairs do not fit the inline pair table (%d)", P, PT_INLINE);
  hipStream_t st = (hipStream_t)stream;
  if (h) LT_HIP(hipSetDevice(h->device));
  if (path < 0 && !d_desc0 && !d_desc1 && !d_s2l0 && !d_s2l1 && !d_dk && !d_match01) {
    // the choice alone, without touching the stream (the matcher additionally needs a scratch slot for the stream: it has one
    // unless PAIR_SLOTS_MAX streams hold them all or the allocation fails)
    if (path_used) {
      const bool fused = P == 1 && fused_pair_applies(dims[0], dims[1], dims[2], dims[3]) && fused_pair_lds_ok();
      *path_used = !fused ? MATCH_THREE : dims[0] == dims[1] && dims[2] == dims[3] ? MATCH_FUSED_IDENT : MATCH_FUSED;
    }
    return LINETR_OK;
  }
  if (!d_desc0 || !d_desc1 || !d_s2l0 || !d_s2l1 || !d_dk || !d_match01 || !d_ws || !off_n0 || !off_n1 || !off_dk || !off_k0)
    return fail(LINETR_E_ARG, "debug_match: null tensor");
  if (((uintptr_t)d_desc0 | (uintptr_t)d_desc1 | (uintptr_t)d_ws) % 16 ||
      ((uintptr_t)d_s2l0 | (uintptr_t)d_s2l1 | (uintptr_t)d_dk | (uintptr_t)d_match01) % 4)
    return fail(LINETR_E_ARG, "debug_match: misaligned tensor (descriptors and workspace 16 bytes, the others 4)");
  MatchForce force;
  force.path = path; force.seg1_global = seg1_global; force.cache_dk = cache_dk; force.device_table = device_table;
  if (int e = match_run(h, P, dims, d_desc0, off_n0, d_s2l0, nullptr, d_desc1, off_n1, d_s2l1, nullptr, thr, mutual, d_dk, off_dk, d_match01,
                        off_k0, d_ws, ws_bytes, stream, force, path_used)) return e;
  LT_HIP(hipStreamSynchronize(st));
  return LINETR_OK;
}

extern "C" int linetr_match_points(LinetrHandle* h, const float* d0_cn, int32_t n0, const float* d1_cn, int32_t n1,
                                   float thr, int32_t mutual, float* d_dist, int32_t* d_match01, void* d_ws,
                                   int64_t ws_bytes, void* stream) {
  if (n0 < 0 || n1 < 0) return fail(LINETR_E_ARG, "match_points: bad argument");
  if (n0 == 0) return LINETR_OK;
  hipStream_t st = (hipStream_t)stream;
  if (h) LT_HIP(hipSetDevice(h->device));
  // scratch: row-major copies + identity sub2line maps + the generic matcher's workspace
  const int64_t need_t = align_up((int64_t)n0 * D * 4, 256) + align_up((int64_t)std::max(n1, 1) * D * 4, 256) +
                         align_up((int64_t)n0 * 4, 256) + align_up((int64_t)std::max(n1, 1) * 4, 256);
  const int64_t need_m = linetr_match_workspace_bytes(1, (int64_t)n0 * n1, 0, n0 + n1);
  if (ws_bytes < need_t + need_m) return fail(LINETR_E_WORKSPACE, "match_points: workspace too small (need %lld)", (long long)(need_t + need_m));
  char* base = (char*)d_ws;
  float* r0 = (float*)base; base += align_up((int64_t)n0 * D * 4, 256);
  float* r1 = (float*)base; base += align_up((int64_t)std::max(n1, 1) * D * 4, 256);
  int* id0 = (int*)base; base += align_up((int64_t)n0 * 4, 256);
  int* id1 = (int*)base; base += align_up((int64_t)std::max(n1, 1) * 4, 256);
  if (!fused_pair_slot(n0, n0, n1, n1, st)) {      // (the one-launch identity path never reads the maps: no upload on the latency path)
    int slot = 0;
    const int m = std::max(n0, n1);
    int* iota = (int*)staging_ring().acquire((size_t)m * sizeof(int), &slot);
    if (!iota) return fail(LINETR_E_HIP, "match_points: pinned staging allocation failed");
    std::iota(iota, iota + m, 0);
    LT_HIP(hipMemcpyAsync(id0, iota, n0 * 4, hipMemcpyHostToDevice, st));
    if (n1 > 0) LT_HIP(hipMemcpyAsync(id1, iota, n1 * 4, hipMemcpyHostToDevice, st));
    if (int e = staging_ring().commit(slot, st)) return e;
  }
  hipLaunchKernelGGL(transpose_cn_kernel, dim3(cdiv(n0, 32), D / 32), dim3(32, 8), 0, st, d0_cn, r0, D, n0);
  if (n1 > 0) hipLaunchKernelGGL(transpose_cn_kernel, dim3(cdiv(n1, 32), D / 32), dim3(32, 8), 0, st, d1_cn, r1, D, n1);
  LT_LAUNCH_CHECK();
  const int32_t dims[4] = {n0, n0, n1, n1};
  const int64_t zero = 0;
  return linetr_match(h, 1, dims, r0, &zero, id0, r1, &zero, id1, thr, mutual, d_dist, &zero, d_match01, &zero, base,
                      ws_bytes - need_t, stream);
}

// The matching tail of Matching.forward (models/matching.py:67-84) in ONE call: point matcher (nn_matcher on the two [256,n] SuperPoint
// descriptor sets), line matcher (get_dist_matrix + subline2keyline + nn_matcher_distmat on the two images' line descriptors) and the
// four device -> host copies of their results into ONE caller-provided pinned block, all asynchronous on `stream`.  Either branch may
// be switched off (np0 = 0 / k0 = 0).  Layout of the pinned block (byte offsets returned in h_offsets[4], every segment 256-aligned):
//   point distances [np0][np1] f32 | point match01 [np0] i32 | key-line distances Dk [k0][k1] f32 | line match01 [k0] i32
namespace {
struct TailLayout { int64_t o_pd, o_pm, o_ld, o_lm, out_total, ws_points, ws_lines, ws_total; };
TailLayout tail_layout(int np0, int np1, int n0, int k0, int n1, int k1) {
  TailLayout L{};
  int64_t o = 0;
  L.o_pd = o; o += align_up((int64_t)np0 * np1 * 4, 256);
  L.o_pm = o; o += align_up((int64_t)np0 * 4, 256);
  L.o_ld = o; o += align_up((int64_t)k0 * k1 * 4, 256);
  L.o_lm = o; o += align_up((int64_t)k0 * 4, 256);
  L.out_total = o;
  L.ws_points = np0 > 0 && np1 > 0 ? 4 * (int64_t)(np0 + np1) * (D + 1) + 2048 + linetr_match_workspace_bytes(1, (int64_t)np0 * np1, 0, np0 + np1) : 0;
  L.ws_lines = k0 > 0 && k1 > 0 ? linetr_match_workspace_bytes(1, (int64_t)n0 * n1, 0, k0 + k1) : 0;
  L.ws_total = align_up(L.out_total, 256) + align_up(L.ws_points, 256) + align_up(L.ws_lines, 256) + 256;
  return L;
}
}  // namespace

extern "C" int64_t linetr_pair_tail_workspace_bytes(int32_t np0, int32_t np1, int32_t n0, int32_t k0, int32_t n1, int32_t k1) {
  return tail_layout(std::max(np0, 0), std::max(np1, 0), std::max(n0, 0), std::max(k0, 0), std::max(n1, 0), std::max(k1, 0)).ws_total;
}

extern "C" int64_t linetr_pair_tail_output_bytes(int32_t np0, int32_t np1, int32_t k0, int32_t k1, int64_t* h_offsets) {
  const TailLayout L = tail_layout(std::max(np0, 0), std::max(np1, 0), 0, std::max(k0, 0), 0, std::max(k1, 0));
  if (h_offsets) { h_offsets[0] = L.o_pd; h_offsets[1] = L.o_pm; h_offsets[2] = L.o_ld; h_offsets[3] = L.o_lm; }
  return L.out_total;
}

extern "C" int linetr_pair_tail(LinetrHandle* h, const float* d_pdesc0_cn, int32_t np0, const float* d_pdesc1_cn, int32_t np1, float thr_p,
                                const float* d_ldesc0, int32_t n0, const int32_t* d_s2l0, int32_t k0, const float* d_ldesc1, int32_t n1,
                                const int32_t* d_s2l1, int32_t k1, float thr_l, int32_t mutual, void* h_pinned_out, int64_t pinned_bytes,
                                void* d_ws, int64_t ws_bytes, void* stream) {
  if (np0 < 0 || np1 < 0 || n0 < 0 || n1 < 0 || k0 < 0 || k1 < 0) return fail(LINETR_E_ARG, "pair_tail: bad dims");
  const bool points = np0 > 0 && np1 > 0, lines = k0 > 0 && k1 > 0;
  const TailLayout L = tail_layout(np0, np1, n0, k0, n1, k1);
  if (!h_pinned_out || pinned_bytes < L.out_total) return fail(LINETR_E_CAPACITY, "pair_tail: output block too small (need %lld)", (long long)L.out_total);
  if (!d_ws || ws_bytes < L.ws_total) return fail(LINETR_E_WORKSPACE, "pair_tail: workspace too small (need %lld)", (long long)L.ws_total);
  hipStream_t st = (hipStream_t)stream;
  if (h) LT_HIP(hipSetDevice(h->device));
  char* dout = (char*)d_ws;                                       // device image of the output block
  char* wsp = dout + align_up(L.out_total, 256);
  char* wsl = wsp + align_up(L.ws_points, 256);
  char* hout = (char*)h_pinned_out;
  if (points) {
    if (!d_pdesc0_cn || !d_pdesc1_cn) return fail(LINETR_E_ARG, "pair_tail: null point descriptors");
    if (int e = linetr_match_points(h, d_pdesc0_cn, np0, d_pdesc1_cn, np1, thr_p, mutual, (float*)(dout + L.o_pd), (int32_t*)(dout + L.o_pm), wsp,
                                    L.ws_points, stream)) return e;
    // requested now: the 1 MB distance matrix travels while the line matcher runs
    LT_HIP(hipMemcpyAsync(hout + L.o_pd, dout + L.o_pd, (size_t)np0 * np1 * 4, hipMemcpyDeviceToHost, st));
    LT_HIP(hipMemcpyAsync(hout + L.o_pm, dout + L.o_pm, (size_t)np0 * 4, hipMemcpyDeviceToHost, st));
  }
  if (lines) {
    if (!d_ldesc0 || !d_ldesc1 || !d_s2l0 || !d_s2l1) return fail(LINETR_E_ARG, "pair_tail: null line descriptors / maps");
    const int32_t dims[4] = {n0, k0, n1, k1};
    const int64_t zero = 0;
    if (int e = linetr_match(h, 1, dims, d_ldesc0, &zero, d_s2l0, d_ldesc1, &zero, d_s2l1, thr_l, mutual, (float*)(dout + L.o_ld), &zero,
                             (int32_t*)(dout + L.o_lm), &zero, wsl, L.ws_lines, stream)) return e;
    LT_HIP(hipMemcpyAsync(hout + L.o_ld, dout + L.o_ld, (size_t)k0 * k1 * 4, hipMemcpyDeviceToHost, st));
    LT_HIP(hipMemcpyAsync(hout + L.o_lm, dout + L.o_lm, (size_t)k0 * 4, hipMemcpyDeviceToHost, st));
  }
  return LINETR_OK;
}

extern "C" int64_t linetr_match_distmat_workspace_bytes(int32_t n0, int32_t n1) {
  n0 = std::max(n0, 0); n1 = std::max(n1, 0);
  return 256 + align_up((int64_t)n0 * 4, 256) + align_up((int64_t)std::max(n1, 1) * 4, 256) +
         align_up((int64_t)n0 * std::max(n1, 1) * 4, 256) + align_up(pair_scratch_ints(n0, n1) * 4, 256);
}

extern "C" int linetr_match_distmat(LinetrHandle* h, const float* d_dist, int32_t n0, int32_t n1, float thr,
                                    int32_t mutual, int32_t* d_match01, void* d_ws, int64_t ws_bytes, void* stream) {
  if (n0 < 0 || n1 < 0) return fail(LINETR_E_ARG, "match_distmat: bad argument");
  if (n0 == 0) return LINETR_OK;
  if (!d_match01 || !d_ws || (n1 > 0 && !d_dist)) return fail(LINETR_E_ARG, "match_distmat: null pointer");
  hipStream_t st = (hipStream_t)stream;
  if (h) LT_HIP(hipSetDevice(h->device));
  // scratch: PairDesc | identity maps | Dk copy | argmin ints
  const int64_t o_id0 = 256, o_id1 = o_id0 + align_up((int64_t)n0 * 4, 256);
  const int64_t o_dk = o_id1 + align_up((int64_t)std::max(n1, 1) * 4, 256);
  const int64_t o_scr = o_dk + align_up((int64_t)n0 * std::max(n1, 1) * 4, 256);
  const int64_t need = linetr_match_distmat_workspace_bytes(n0, n1);
  if (!d_ws || ws_bytes < need) return fail(LINETR_E_WORKSPACE, "match_distmat: workspace too small (need %lld)", (long long)need);
  char* base = (char*)d_ws;
  const int m = std::max(n0, n1);
  int slot = 0;
  int* iota = (int*)staging_ring().acquire((size_t)m * sizeof(int), &slot);
  if (!iota) return fail(LINETR_E_HIP, "match_distmat: pinned staging allocation failed");
  PairTable tab{};
  tab.n_inline = 1;
  PairDesc* pd = tab.inl;
  pd->n0 = pd->k0 = n0; pd->n1 = pd->k1 = n1;
  pd->chunks = cdiv(n0, PM_ROWS);
  std::iota(iota, iota + m, 0);
  LT_HIP(hipMemcpyAsync(base + o_id0, iota, n0 * 4, hipMemcpyHostToDevice, st));
  if (n1 > 0) LT_HIP(hipMemcpyAsync(base + o_id1, iota, n1 * 4, hipMemcpyHostToDevice, st));
  if (int e = staging_ring().commit(slot, st)) return e;
  if (n1 > 0) {
    const int seg1_global = n1 > PM_MAX_K1;
    if (seg1_global) {
      hipLaunchKernelGGL(pair_seg1_kernel, dim3(cdiv(n1, 2048), 1), dim3(256), 0, st, tab, (const int*)(base + o_id1), (int*)(base + o_scr));
      LT_LAUNCH_CHECK();
    }
    const int cache_dk = n1 <= PM_CACHE_K1;
    hipLaunchKernelGGL(pair_pool_kernel, dim3(pd->chunks, 1), dim3(256), pair_pool_lds(n1, seg1_global, cache_dk),
                       st, tab, (const int*)(base + o_id0), (const int*)(base + o_id1), d_dist, (float*)(base + o_dk),
                       (int*)(base + o_scr), seg1_global, cache_dk);
    LT_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(pair_final_kernel, dim3(1), dim3(256), 0, st, tab, thr, mutual, d_match01, (int*)(base + o_scr));
  LT_LAUNCH_CHECK();
  return LINETR_OK;
}

extern "C" int64_t linetr_match_distmat_f64_workspace_bytes(int32_t n0, int32_t n1) {
  n0 = std::max(n0, 0); n1 = std::max(n1, 0);
  return align_up((int64_t)n0 * 8, 256) + align_up((int64_t)n0 * 4, 256) + align_up((int64_t)std::max(n1, 1) * 4, 256) + 256;
}

extern "C" int linetr_match_distmat_f64(LinetrHandle* h, const double* d_dist, int32_t n0, int32_t n1, double thr, int32_t mutual,
                                        int32_t* d_match01, void* d_ws, int64_t ws_bytes, void* stream) {
  if (n0 < 0 || n1 < 0) return fail(LINETR_E_ARG, "match_distmat_f64: bad argument");
  if (n0 == 0) return LINETR_OK;
  if (!d_match01 || !d_ws || (n1 > 0 && !d_dist)) return fail(LINETR_E_ARG, "match_distmat_f64: null pointer");
  if (ws_bytes < linetr_match_distmat_f64_workspace_bytes(n0, n1)) return fail(LINETR_E_WORKSPACE, "match_distmat_f64: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  if (h) LT_HIP(hipSetDevice(h->device));
  if (n1 == 0) { LT_HIP(hipMemsetAsync(d_match01, 0xff, (size_t)n0 * 4, st)); return LINETR_OK; }
  char* base = (char*)d_ws;
  double* row_min = (double*)base;
  int* row_arg = (int*)(base + align_up((int64_t)n0 * 8, 256));
  int* col_arg = (int*)((char*)row_arg + align_up((int64_t)n0 * 4, 256));
  hipLaunchKernelGGL(argmin_rows_f64_kernel, dim3(cdiv(n0, 4)), dim3(256), 0, st, d_dist, n0, n1, row_arg, row_min);
  hipLaunchKernelGGL(argmin_cols_f64_kernel, dim3(cdiv(n1, 256)), dim3(256), 0, st, d_dist, n0, n1, col_arg);
  hipLaunchKernelGGL(match_final_f64_kernel, dim3(cdiv(n0, 256)), dim3(256), 0, st, (const int*)row_arg, (const double*)row_min,
                     (const int*)col_arg, n0, thr, mutual, d_match01);
  LT_LAUNCH_CHECK();
  return LINETR_OK;
}

// subline2keyline (models/line_transformer.py:277-282) alone: Dk = A0 D A1^T for the segmented-mean matrices the tokeniser
// produces, given as sub-line -> key-line maps (non-decreasing).  Same kernel as linetr_match's pooling stage.
extern "C" int64_t linetr_pool_distmat_workspace_bytes(int32_t k0, int32_t k1) {
  return align_up(pair_scratch_ints(std::max(k0, 0), std::max(k1, 0)) * 4, 256) + 256;
}

extern "C" int linetr_pool_distmat(LinetrHandle* h, const float* d_dist, int32_t n0, int32_t n1, const int32_t* d_s2l0, int32_t k0,
                                   const int32_t* d_s2l1, int32_t k1, float* d_dk, void* d_ws, int64_t ws_bytes, void* stream) {
  if (n0 < 0 || n1 < 0 || k0 < 0 || k1 < 0 || k0 > n0 || k1 > n1) return fail(LINETR_E_ARG, "pool_distmat: bad dims");
  if (k0 == 0 || k1 == 0) return LINETR_OK;
  if (!d_dist || !d_s2l0 || !d_s2l1 || !d_dk || !d_ws) return fail(LINETR_E_ARG, "pool_distmat: null pointer");
  if (ws_bytes < linetr_pool_distmat_workspace_bytes(k0, k1)) return fail(LINETR_E_WORKSPACE, "pool_distmat: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  if (h) LT_HIP(hipSetDevice(h->device));
  PairTable tab{};
  tab.n_inline = 1;
  PairDesc* pd = tab.inl;
  pd->n0 = n0; pd->k0 = k0; pd->n1 = n1; pd->k1 = k1;
  pd->chunks = cdiv(k0, PM_ROWS);
  const int seg1_global = k1 > PM_MAX_K1;
  ProfScope ps(h, st, "pair_pool", 0, 4.0 * ((double)n0 * n1 + (double)k0 * k1));
  if (seg1_global) {
    hipLaunchKernelGGL(pair_seg1_kernel, dim3(cdiv(n1, 2048), 1), dim3(256), 0, st, tab, d_s2l1, (int*)d_ws);
    LT_LAUNCH_CHECK();
  }
  const int cache_dk = k1 <= PM_CACHE_K1;
  hipLaunchKernelGGL(pair_pool_kernel, dim3(pd->chunks, 1), dim3(256), pair_pool_lds(k1, seg1_global, cache_dk), st,
                     tab, d_s2l0, d_s2l1, d_dist, d_dk, (int*)d_ws, seg1_global, cache_dk);
  LT_LAUNCH_CHECK();
  return LINETR_OK;
}

// subline2keyline on the two mat_klines2sublines MATRICES, as the reference's call sites hand them over (models/matching.py:80:
// data['mat_klines2sublines0'][0], a [K,N] float32 tensor).  A tokeniser's matrix is reduced to its sub-line -> key-line map on the
// device and pooled by the segmented-mean kernel; any other matrix is multiplied out as given.  Asynchronous on `stream`.
namespace {
struct DensePoolLayout { int64_t o_map0, o_map1, o_val0, o_val1, o_verdict, o_tmp, o_pool, total; };
DensePoolLayout dense_pool_layout(int k0, int n0, int k1, int n1) {
  DensePoolLayout L{};
  int64_t o = 0;
  L.o_verdict = o; o += 256;                         // FIRST: the header promises the verdict word at the workspace's offset 0
  L.o_map0 = o; o += align_up((int64_t)std::max(n0, 1) * 4, 256);
  L.o_map1 = o; o += align_up((int64_t)std::max(n1, 1) * 4, 256);
  L.o_val0 = o; o += align_up((int64_t)std::max(n0, 1) * 4, 256);
  L.o_val1 = o; o += align_up((int64_t)std::max(n1, 1) * 4, 256);
  L.o_tmp = o; o += align_up((int64_t)std::max(k0, 1) * std::max(n1, 1) * 4, 256);
  L.o_pool = o; o += linetr_pool_distmat_workspace_bytes(std::min(k0, n0), std::min(k1, n1));
  L.total = o;
  return L;
}
}  // namespace

extern "C" int64_t linetr_pool_distmat_dense_workspace_bytes(int32_t k0, int32_t n0, int32_t k1, int32_t n1) {
  return dense_pool_layout(std::max(k0, 0), std::max(n0, 0), std::max(k1, 0), std::max(n1, 0)).total;
}

extern "C" int linetr_pool_distmat_dense(LinetrHandle* h, const float* d_dist, int32_t n0, int32_t n1, const float* d_A0, int32_t k0,
                                         const float* d_A1, int32_t k1, float* d_dk, void* d_ws, int64_t ws_bytes, void* stream) {
  if (n0 < 0 || n1 < 0 || k0 < 0 || k1 < 0) return fail(LINETR_E_ARG, "pool_distmat_dense: bad dims");
  if (k0 > 65535) return fail(LINETR_E_ARG, "pool_distmat_dense: more than 65535 key-lines in image 0 (grid limit of the as-given product)");
  if (k0 == 0 || k1 == 0) return LINETR_OK;
  if (!d_dk || !d_ws || ((n0 > 0 && n1 > 0) && (!d_dist || !d_A0 || !d_A1))) return fail(LINETR_E_ARG, "pool_distmat_dense: null pointer");
  const DensePoolLayout L = dense_pool_layout(k0, n0, k1, n1);
  if (ws_bytes < L.total) return fail(LINETR_E_WORKSPACE, "pool_distmat_dense: workspace too small (need %lld)", (long long)L.total);
  hipStream_t st = (hipStream_t)stream;
  if (h) LT_HIP(hipSetDevice(h->device));
  char* base = (char*)d_ws;
  int* verdict = (int*)(base + L.o_verdict);
  if (n0 == 0 || n1 == 0) {                          // an empty inner dimension: the product is a zero matrix
    LT_HIP(hipMemsetAsync(d_dk, 0, (size_t)k0 * k1 * 4, st));
    return LINETR_OK;
  }
  // K > N cannot be a tokeniser's matrix (every key-line owns at least one sub-line): the verdict starts non-zero and the
  // segmented-mean launch is skipped
  const bool poolable = k0 <= n0 && k1 <= n1;
  LT_HIP(hipMemsetD32Async((hipDeviceptr_t)verdict, poolable ? 0 : 1, 1, st));   // the WORD 1 (a byte-wise memset left 0x01010101 for a reader of the verdict)
  if (poolable) {
    int* map0 = (int*)(base + L.o_map0); int* map1 = (int*)(base + L.o_map1);
    float* val0 = (float*)(base + L.o_val0); float* val1 = (float*)(base + L.o_val1);
    hipLaunchKernelGGL(mat_to_map_kernel, dim3(cdiv(n0, 256)), dim3(256), 0, st, d_A0, k0, n0, map0, val0, verdict);
    hipLaunchKernelGGL(mat_to_map_kernel, dim3(cdiv(n1, 256)), dim3(256), 0, st, d_A1, k1, n1, map1, val1, verdict);
    hipLaunchKernelGGL(mat_check_kernel, dim3(cdiv(n0, 256)), dim3(256), 0, st, (const int*)map0, (const float*)val0, k0, n0, verdict);
    hipLaunchKernelGGL(mat_check_kernel, dim3(cdiv(n1, 256)), dim3(256), 0, st, (const int*)map1, (const float*)val1, k1, n1, verdict);
    hipLaunchKernelGGL(map_sanitize_kernel, dim3(cdiv(n0, 256)), dim3(256), 0, st, map0, k0, n0, (const int*)verdict);
    hipLaunchKernelGGL(map_sanitize_kernel, dim3(cdiv(n1, 256)), dim3(256), 0, st, map1, k1, n1, (const int*)verdict);
    LT_LAUNCH_CHECK();
    if (int e = linetr_pool_distmat(h, d_dist, n0, n1, map0, k0, map1, k1, d_dk, base + L.o_pool, ws_bytes - L.o_pool, stream)) return e;
  }
  float* tmp = (float*)(base + L.o_tmp);
  hipLaunchKernelGGL(dense_pool_left_kernel, dim3(cdiv(n1, 256), k0), dim3(256), 0, st, d_A0, d_dist, tmp, n0, n1, (const int*)verdict);
  hipLaunchKernelGGL(dense_pool_right_kernel, dim3(cdiv(k1, 4), k0), dim3(256), 0, st, (const float*)tmp, d_A1, d_dk, n1, k1, (const int*)verdict);
  LT_LAUNCH_CHECK();
  return LINETR_OK;
}

// One rank's all-gather slab in one launch (layout: lt_match.h pack_slab_kernel, linetr_amd/parallel.py)
extern "C" int linetr_pack_slab(const float* d_line_desc, int32_t N, const int32_t* d_cu_n, const int32_t* d_cu_k, int32_t n_images,
                                const int32_t* d_sub2line, int32_t n_images_cap, int32_t rows_cap, int32_t zero_tail, float* d_slab,
                                void* stream) {
  if (N < 0 || n_images < 0 || n_images > n_images_cap || N > rows_cap) return fail(LINETR_E_CAPACITY, "pack_slab: %d images / %d rows exceed the slab capacity (%d / %d)", n_images, N, n_images_cap, rows_cap);
  if (!d_slab || (N > 0 && !d_line_desc) || (n_images > 0 && !d_cu_n)) return fail(LINETR_E_ARG, "pack_slab: null pointer");
  const int hr = (1 + 2 * n_images_cap + D - 1) / D, mr = (rows_cap + D - 1) / D;
  const int64_t items = (int64_t)(zero_tail ? rows_cap : N) * (D / 4) + (d_sub2line ? N : 0) + 1 + 2 * (int64_t)n_images_cap;
  hipLaunchKernelGGL(pack_slab_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_line_desc, N, d_cu_n,
                     d_cu_k, n_images, d_sub2line, n_images_cap, rows_cap, hr, mr, zero_tail, d_slab);
  LT_LAUNCH_CHECK();
  return LINETR_OK;
}

extern "C" int linetr_superpoint_heads(LinetrHandle* h, const float* d_score_logits, const float* d_desc_raw, int32_t B,
                                       int32_t Hc, int32_t Wc, float* d_dense_score, float* d_dense_desc_nhwc,
                                       float* d_dense_desc_nchw, void* stream) {
  if (B < 0 || Hc <= 0 || Wc <= 0) return fail(LINETR_E_ARG, "superpoint_heads: bad shape B=%d Hc=%d Wc=%d", B, Hc, Wc);
  if (d_dense_score && !d_score_logits) return fail(LINETR_E_ARG, "superpoint_heads: score output without score logits");
  if ((d_dense_desc_nhwc || d_dense_desc_nchw) && !d_desc_raw)
    return fail(LINETR_E_ARG, "superpoint_heads: descriptor output without the raw descriptor head");
  if (B == 0) return LINETR_OK;
  if (h) LT_HIP(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  const int HW = Hc * Wc;
  const dim3 grid((unsigned)cdiv(HW, 64), (unsigned)B);
  if (d_dense_desc_nhwc || d_dense_desc_nchw) {
    const double by = (double)B * HW * D * 4.0 * (1 + (d_dense_desc_nhwc ? 1 : 0) + (d_dense_desc_nchw ? 1 : 0));
    ProfScope ps(h, st, "sp_desc_head", 3.0 * B * HW * D, by);
    hipLaunchKernelGGL(sp_desc_head_kernel<32>, dim3((unsigned)cdiv(HW, 32), (unsigned)B), dim3(256), 0, st, d_desc_raw, d_dense_desc_nhwc, d_dense_desc_nchw, HW);
    LT_LAUNCH_CHECK();
  }
  if (d_dense_score) {
    ProfScope ps(h, st, "sp_score_head", 0, (double)B * HW * (65 + 64) * 4.0);
    hipLaunchKernelGGL(sp_score_head_kernel, grid, dim3(256), 0, st, d_score_logits, d_dense_score, Hc, Wc);
    LT_LAUNCH_CHECK();
  }
  return LINETR_OK;
}

// =============================================================================================
// SuperPoint key-point branch (lt_keypoints.h)
// =============================================================================================

namespace {
// workspace of linetr_superpoint_keypoints: bit mask | per-row offsets | top-k candidate keys
struct KpLayout { int Wm; int64_t o_mask, o_rowoff, o_keys, total; };
KpLayout kp_layout(int B, int H, int W, int cap) {
  KpLayout L{};
  L.Wm = cdiv(W, 32);
  int64_t o = 0;
  L.o_mask = o; o += align_up((int64_t)B * H * L.Wm * 4, 256);
  L.o_rowoff = o; o += align_up((int64_t)B * H * 4, 256);
  L.o_keys = o; o += align_up((int64_t)B * cap * 8, 256);
  L.total = o + 256;
  return L;
}

// sp_nms_kernel takes more than 64 KiB of dynamic LDS: raised once per device
bool kp_lds_ok() { return allow_dynamic_lds<sp_nms_kernel>((int)kp_nms_lds(KP_MAX_R)) == hipSuccess; }
}  // namespace

extern "C" int64_t linetr_superpoint_keypoints_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t cap_per_image) {
  return kp_layout(std::max(B, 0), std::max(H, 0), std::max(W, 0), std::max(cap_per_image, 0)).total;
}

extern "C" int linetr_superpoint_keypoints(LinetrHandle* h, const float* d_dense_score, int32_t B, int32_t H, int32_t W, int32_t nms_radius,
                                           float keypoint_threshold, int32_t remove_borders, int32_t max_keypoints, int32_t cap_per_image,
                                           float* d_keypoints, float* d_scores, int32_t* d_cu_kp, int32_t* d_found, void* d_ws,
                                           int64_t ws_bytes, void* stream) {
  if (B < 0 || H <= 0 || W <= 0 || cap_per_image < 0 || (int64_t)H * W > INT32_MAX || (int64_t)B * H > INT32_MAX)
    return fail(LINETR_E_ARG, "superpoint_keypoints: bad shape B=%d H=%d W=%d cap=%d", B, H, W, cap_per_image);
  if (nms_radius < 0 || nms_radius > KP_MAX_R) return fail(LINETR_E_ARG, "superpoint_keypoints: nms_radius %d outside 0..%d", nms_radius, KP_MAX_R);
  if (max_keypoints < -1 || max_keypoints == 0 || max_keypoints > KP_MAX_K)
    return fail(LINETR_E_ARG, "superpoint_keypoints: max_keypoints %d (need -1 or 1..%d)", max_keypoints, KP_MAX_K);
  // suppressed pixels hold 0 in the reference's map: with a threshold below 0 they would all be key points
  if (!(keypoint_threshold >= 0.f)) return fail(LINETR_E_ARG, "superpoint_keypoints: keypoint_threshold must be >= 0");
  if (remove_borders < 0) return fail(LINETR_E_ARG, "superpoint_keypoints: remove_borders must be >= 0");
  if (!d_cu_kp || (B > 0 && (!d_dense_score || !d_found || !d_ws || (cap_per_image > 0 && (!d_keypoints || !d_scores)))))
    return fail(LINETR_E_ARG, "superpoint_keypoints: null pointer");
  hipStream_t st = (hipStream_t)stream;
  if (h) LT_HIP(hipSetDevice(h->device));
  if (B == 0) { LT_HIP(hipMemsetAsync(d_cu_kp, 0, 4, st)); return LINETR_OK; }
  const KpLayout L = kp_layout(B, H, W, cap_per_image);
  if (ws_bytes < L.total) return fail(LINETR_E_WORKSPACE, "superpoint_keypoints: workspace too small (need %lld)", (long long)L.total);
  if (!kp_lds_ok()) return fail(LINETR_E_HIP, "superpoint_keypoints: the device refuses the kernels' dynamic LDS");
  char* base = (char*)d_ws;
  unsigned* mask = (unsigned*)(base + L.o_mask);
  int* row_off = (int*)(base + L.o_rowoff);
  unsigned long long* keys = max_keypoints >= 0 ? (unsigned long long*)(base + L.o_keys) : nullptr;
  const int r = nms_radius, TH = kp_tile_h(r);
  const double map_bytes = (double)B * H * W * 4, mask_bytes = (double)B * H * L.Wm * 4;
  {
    ProfScope ps(h, st, "sp_nms", 0, map_bytes + mask_bytes);
    hipLaunchKernelGGL(sp_nms_kernel, dim3((unsigned)cdiv(W, KP_TW), (unsigned)cdiv(H, TH), (unsigned)B), dim3(256), kp_nms_lds(r), st,
                       d_dense_score, H, W, r, TH, keypoint_threshold, remove_borders, mask, L.Wm);
    LT_LAUNCH_CHECK();
  }
  {
    ProfScope ps(h, st, "sp_kp_compact", 0, 2 * mask_bytes + 3.0 * B * H * 4);
    hipLaunchKernelGGL(sp_kp_scan_kernel, dim3((unsigned)B), dim3(256), 0, st, (const unsigned*)mask, H, L.Wm, row_off, d_found);
    hipLaunchKernelGGL(sp_kp_offsets_kernel, dim3(1), dim3(256), 0, st, (const int*)d_found, B, cap_per_image, max_keypoints, d_cu_kp);
    hipLaunchKernelGGL(sp_kp_emit_kernel, dim3((unsigned)(((int64_t)B * H + 3) / 4)), dim3(256), 0, st, d_dense_score, (const unsigned*)mask,
                       (const int*)row_off, (const int*)d_cu_kp, (int64_t)B * H, H, W, L.Wm, cap_per_image, d_keypoints, d_scores, keys);
    LT_LAUNCH_CHECK();
  }
  if (keys) {
    ProfScope ps(h, st, "sp_kp_topk", 0, (double)B * cap_per_image * 8);
    hipLaunchKernelGGL(sp_kp_topk_kernel, dim3((unsigned)B), dim3(512), 0, st, (const unsigned long long*)keys, (const int*)d_found,
                       (const int*)d_cu_kp, cap_per_image, max_keypoints, W, d_keypoints, d_scores);
    LT_LAUNCH_CHECK();
  }
  return LINETR_OK;
}

// =============================================================================================
// validation step (lt_valstep.h)
// =============================================================================================

namespace {
constexpr int VS_MAX_N = 32768;   // n^2 dot products per item are indexed in 64 bits; the grids stay far inside their limits
constexpr int VS_MAX_B = 65535;   // grid.z / grid.y
struct ValOutLayout { int64_t o_scalars, o_count, o_counts, o_scores, total; };
ValOutLayout val_out_layout(int B) {
  ValOutLayout L{};
  int64_t o = 0;
  L.o_scalars = o; o += 256;
  L.o_count = o; o += 256;
  L.o_counts = o; o += align_up((int64_t)B * 4 * 4, 256);
  L.o_scores = o; o += align_up((int64_t)B * 3 * 8, 256);
  L.total = o;
  return L;
}
// workspace: device image of the result block | dots | norms | per-row results | argmins | match01
struct ValWsLayout { int64_t o_out, o_dots, o_sq0, o_sq1, o_pos, o_neg, o_rarg, o_rmin, o_carg, o_gt, o_m01, total; };
ValWsLayout val_ws_layout(int B, int n) {
  ValWsLayout L{};
  const int64_t rows = align_up((int64_t)B * n * 4, 256);
  int64_t o = 0;
  L.o_out = o; o += val_out_layout(B).total;
  L.o_dots = o; o += align_up((int64_t)B * n * n * 4, 256);
  L.o_sq0 = o; o += rows;
  L.o_sq1 = o; o += rows;
  L.o_pos = o; o += 2 * rows;
  L.o_neg = o; o += 2 * rows;
  L.o_rarg = o; o += rows;
  L.o_rmin = o; o += rows;
  L.o_carg = o; o += rows;
  L.o_gt = o; o += rows;
  L.o_m01 = o; o += rows;
  L.total = o + 256;
  return L;
}
bool val_dims_ok(int B, int n) { return B > 0 && B <= VS_MAX_B && n > 0 && n <= VS_MAX_N; }
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
  // every refusal comes before the first launch
  if (n0 != n1) return fail(LINETR_E_ARG, "val_step: %d and %d sub-lines (the criterion stacks D on D^T: one n for both sides)", n0, n1);
  const int n = n0;
  if (!val_dims_ok(B, n)) return fail(LINETR_E_ARG, "val_step: bad shape B=%d n=%d (B 1..%d, n 1..%d)", B, n, VS_MAX_B, VS_MAX_N);
  if (!d_desc0 || !d_desc1 || !d_assign || !h_pinned_out || !d_ws) return fail(LINETR_E_ARG, "val_step: null pointer");
  const ValOutLayout O = val_out_layout(B);
  const ValWsLayout W = val_ws_layout(B, n);
  if (pinned_bytes < O.total) return fail(LINETR_E_ARG, "val_step: output block too small (need %lld)", (long long)O.total);
  if (ws_bytes < W.total) return fail(LINETR_E_ARG, "val_step: workspace too small (need %lld)", (long long)W.total);
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
  const int tiles = cdiv(n, 64);
  {
    ProfScope ps(h, st, "val_dot", 2.0 * B * n * n * D, 4.0 * B * (2.0 * n * D + (double)n * n));
    hipLaunchKernelGGL(val_dot_kernel, dim3(tiles, tiles, B), dim3(256), 0, st, d_desc0, d_desc1, n, dots, sq0, sq1);
    LT_LAUNCH_CHECK();
  }
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
  int64_t o = 0;
  L.o_out = o; o += 256;
  L.o_dots = o; o += align_up((int64_t)B * n * n * 4, 256);
  L.o_sq0 = o; o += rows;
  L.o_sq1 = o; o += rows;
  L.o_pos = o; o += 2 * rows;
  L.o_neg = o; o += 2 * rows;
  L.o_ties = o; o += 2 * rows;
  L.o_arg = o; o += 2 * rows;
  L.total = o + 256;
  return L;
}
}  // namespace

extern "C" int64_t linetr_desc_loss_grad_workspace_bytes(int32_t B, int32_t n) {
  return val_dims_ok(B, n) ? loss_grad_ws_layout(B, n).total : 0;
}

extern "C" int linetr_desc_loss_grad(LinetrHandle* h, const float* d_desc0, int32_t n0, const float* d_desc1, int32_t n1, const float* d_assign,
                                     int32_t B, const float* d_upstream, float* d_grad0, float* d_grad1, void* h_pinned_out,
                                     int64_t pinned_bytes, void* d_ws, int64_t ws_bytes, void* stream) {
  // every refusal comes before the first launch
  if (n0 != n1) return fail(LINETR_E_ARG, "desc_loss_grad: %d and %d sub-lines (the criterion stacks D on D^T: one n for both sides)", n0, n1);
  const int n = n0;
  if (!val_dims_ok(B, n)) return fail(LINETR_E_ARG, "desc_loss_grad: bad shape B=%d n=%d (B 1..%d, n 1..%d)", B, n, VS_MAX_B, VS_MAX_N);
  if (!d_desc0 || !d_desc1 || !d_assign || !h_pinned_out || !d_ws) return fail(LINETR_E_ARG, "desc_loss_grad: null pointer");
  const LossGradWsLayout W = loss_grad_ws_layout(B, n);
  if (pinned_bytes < LG_OUT_BYTES) return fail(LINETR_E_ARG, "desc_loss_grad: output block too small (need %lld)", (long long)LG_OUT_BYTES);
  if (ws_bytes < W.total) return fail(LINETR_E_ARG, "desc_loss_grad: workspace too small (need %lld)", (long long)W.total);
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
  const int tiles = cdiv(n, 64);
  {
    ProfScope ps(h, st, "val_dot", 2.0 * B * n * n * D, 4.0 * B * (2.0 * n * D + (double)n * n));
    hipLaunchKernelGGL(val_dot_kernel, dim3(tiles, tiles, B), dim3(256), 0, st, d_desc0, d_desc1, n, dots, (float*)(base + W.o_sq0),
                       (float*)(base + W.o_sq1));
    LT_LAUNCH_CHECK();
  }
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
    hipLaunchKernelGGL(lg_grad_kernel, dim3(tiles, 2, B), dim3(256), 0, st, d_desc0, d_desc1, (const float*)dots, d_assign, n,
                       (const float*)row_pos, (const int*)row_ties, (const int*)row_arg, (const long long*)count, d_upstream, d_grad0, d_grad1);
    LT_LAUNCH_CHECK();
  }
  LT_HIP(hipMemcpyAsync(h_pinned_out, scalars, (size_t)LG_OUT_BYTES, hipMemcpyDeviceToHost, st));
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
  int64_t o = 0;
  L.o_dw = o; o += align_up((int64_t)L.chunks * N * K * 4, 256);
  L.o_db = o; o += align_up((int64_t)L.chunks * N * 4, 256);
  L.total = o + 256;
  return L;
}
bool lin_dims_ok(int64_t rows, int N, int K) {
  return rows >= 1 && rows <= LB_MAX_ROWS && N > 0 && K > 0 && N % 64 == 0 && K % 32 == 0 && N <= 1024 && K <= 1024;
}
bool lin_stride_ok(int64_t ld, int width) { return ld >= width && ld % 4 == 0; }
bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }     // (NULL passes: an absent optional pointer)

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
unsigned attn_tiles(int64_t N, int n_images) { return (unsigned)(N / AB_T + n_images); }
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
// ground-truth line assignment of a homography pair (lt_gtassign.h)
// =============================================================================================

namespace {
// workspace (sized for the double instance): projected lines of both sides | the four angle arrays | ballot words | found
struct GtLayout { int W64; int64_t o_proj0, o_proj1, o_ang, o_words, o_found, total; };
GtLayout gt_layout(int B, int n0, int n1) {
  GtLayout L{};
  L.W64 = cdiv(n1, 64);
  int64_t o = 0;
  L.o_proj0 = o; o += align_up((int64_t)B * n0 * 4 * 8, 256);
  L.o_proj1 = o; o += align_up((int64_t)B * n1 * 4 * 8, 256);
  L.o_ang = o; o += align_up((int64_t)B * 2 * ((int64_t)n0 + n1) * 8, 256);
  L.o_words = o; o += align_up((int64_t)B * n0 * L.W64 * 8, 256);
  L.o_found = o; o += align_up((int64_t)B * 4, 256);
  L.total = o + 256;
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
