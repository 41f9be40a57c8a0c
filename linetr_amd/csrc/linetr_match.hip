// liblinetr_hip.so, translation unit 3 of 6: the descriptor-distance matcher, the dense-map producer and the slab packing of the
// multi-GPU path (C ABI in include/linetr_hip.h; kernels in lt_match.h, lt_producer.h) and SuperPoint's key-point branch
// (lt_keypoints.h).  Training and evaluation are linetr_train.hip.
#include <algorithm>
#include <numeric>

#include "lt_handle.h"
#include "lt_match.h"
#include "lt_producer.h"
#include "lt_keypoints.h"

using namespace lt;

// =============================================================================================
// matcher
// =============================================================================================

namespace {
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
int64_t pair_scratch_ints(int k0, int k1) { return sz_add(2 * (int64_t)k0 + 2 * (int64_t)k1 + 1, sz_mul(2 * (int64_t)cdiv(std::max(k0, 1), PM_ROWS), k1), 8); }

// workspace of linetr_match / linetr_match_gathered: device pair table | distance matrices | argmin scratch
struct MatchLayout { int64_t o_table, o_dist, o_scratch, total; };
MatchLayout match_layout(int P, int64_t sum_n0n1, int64_t sum_k) {
  MatchLayout L{};
  Carve c;
  L.o_table = c.take(sz_mul(P, sizeof(PairDesc)));
  L.o_dist = c.take(sz_mul(sum_n0n1, 4));
  // scratch bound: sum over pairs of pair_scratch_ints(k0,k1) <= 4 sum_k + 2 (sum_k0k1 / PM_ROWS + sum_k) + 9 P, and
  // k0 k1 <= n0 n1
  L.o_scratch = c.take(sz_mul(sz_add(sz_mul(6, sum_k), 2 * (sum_n0n1 / PM_ROWS + 1), sz_mul(9, P)), 4));
  L.total = sz_add(c.o, 256);
  return L;
}
}  // namespace

extern "C" int64_t linetr_match_workspace_bytes(int32_t n_pairs, int64_t sum_n0n1, int64_t sum_k0k1, int64_t sum_k) {
  (void)sum_k0k1;
  return sz_answer(match_layout(n_pairs, sum_n0n1, sum_k).total);
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

// The pooling stage of the P pairs of `tab`: the segment table of side 1 in d_scr where max_k1 key-lines do not fit the LDS, then
// pair_pool_kernel.  seg1_global / cache_dk: MatchForce's two choices (-1: decided here).
int pool_stage(hipStream_t st, const PairTable& tab, int P, int max_n1, int max_k1, int max_chunks, const int* d_s2l0, const int* d_s2l1,
               const float* d_dist, float* d_dk, int* d_scr, int seg1_global = -1, int cache_dk = -1) {
  if (seg1_global < 0) seg1_global = max_k1 > PM_MAX_K1;    // the reference has no limit (max_keylines / max_keypoints = -1)
  if (seg1_global) {
    hipLaunchKernelGGL(pair_seg1_kernel, dim3(cdiv(max_n1, 2048), P), dim3(256), 0, st, tab, d_s2l1, d_scr);
    LT_LAUNCH_CHECK();
  }
  if (cache_dk < 0) cache_dk = max_k1 <= PM_CACHE_K1;
  hipLaunchKernelGGL(pair_pool_kernel, dim3(max_chunks, P), dim3(256), pair_pool_lds(max_k1, seg1_global, cache_dk), st, tab, d_s2l0,
                     d_s2l1, d_dist, d_dk, d_scr, seg1_global, cache_dk);
  LT_LAUNCH_CHECK();
  return LINETR_OK;
}

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
  const MatchLayout L = match_layout(P, od, sum_k);
  if (ws_bytes < L.total) return fail(LINETR_E_WORKSPACE, "match: workspace too small");
  char* base = (char*)d_ws;
  PairDesc* d_pd = (PairDesc*)(base + L.o_table);
  float* d_dist = (float*)(base + L.o_dist);
  int* d_scr = (int*)(base + L.o_scratch);
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
    if (max_k1 > 0)
      if (int e = pool_stage(st, tab, P, max_n1, max_k1, max_chunks, d_s2l0, d_s2l1, d_dist, d_dk, d_scr, force.seg1_global, force.cache_dk))
        return e;
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

namespace {
// workspace of linetr_match_points: row-major copies | identity sub2line maps | the generic matcher's workspace
struct PointsLayout { int64_t o_r0, o_r1, o_id0, o_id1, o_match, match_bytes, total; };
PointsLayout points_layout(int n0, int n1) {
  PointsLayout L{};
  Carve c;
  L.o_r0 = c.take((int64_t)n0 * D * 4);
  L.o_r1 = c.take((int64_t)std::max(n1, 1) * D * 4);
  L.o_id0 = c.take((int64_t)n0 * 4);
  L.o_id1 = c.take((int64_t)std::max(n1, 1) * 4);
  L.match_bytes = match_layout(1, (int64_t)n0 * n1, (int64_t)n0 + n1).total;
  L.o_match = c.take(L.match_bytes);
  L.total = c.o;
  return L;
}
}  // namespace

extern "C" int64_t linetr_match_points_workspace_bytes(int32_t n0, int32_t n1) {
  return sz_answer(points_layout(std::max(n0, 0), std::max(n1, 0)).total);
}

extern "C" int linetr_match_points(LinetrHandle* h, const float* d0_cn, int32_t n0, const float* d1_cn, int32_t n1,
                                   float thr, int32_t mutual, float* d_dist, int32_t* d_match01, void* d_ws,
                                   int64_t ws_bytes, void* stream) {
  if (n0 < 0 || n1 < 0) return fail(LINETR_E_ARG, "match_points: bad argument");
  if (n0 == 0) return LINETR_OK;
  hipStream_t st = (hipStream_t)stream;
  if (h) LT_HIP(hipSetDevice(h->device));
  const PointsLayout L = points_layout(n0, n1);
  if (ws_bytes < L.total) return fail(LINETR_E_WORKSPACE, "match_points: workspace too small (need %lld)", (long long)L.total);
  char* base = (char*)d_ws;
  float *r0 = (float*)(base + L.o_r0), *r1 = (float*)(base + L.o_r1);
  int *id0 = (int*)(base + L.o_id0), *id1 = (int*)(base + L.o_id1);
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
  return linetr_match(h, 1, dims, r0, &zero, id0, r1, &zero, id1, thr, mutual, d_dist, &zero, d_match01, &zero, base + L.o_match,
                      L.match_bytes, stream);
}

// The matching tail of Matching.forward (models/matching.py:67-84) in ONE call: point matcher (nn_matcher on the two [256,n] SuperPoint
// descriptor sets), line matcher (get_dist_matrix + subline2keyline + nn_matcher_distmat on the two images' line descriptors) and the
// four device -> host copies of their results into ONE caller-provided pinned block, all asynchronous on `stream`.  Either branch may
// be switched off (np0 = 0 / k0 = 0).  Layout of the pinned block (byte offsets returned in h_offsets[4], every segment 256-aligned):
//   point distances [np0][np1] f32 | point match01 [np0] i32 | key-line distances Dk [k0][k1] f32 | line match01 [k0] i32
namespace {
// (the workspace: device image of the output block, at offset 0 | the point matcher's | the line matcher's)
struct TailLayout { int64_t o_pd, o_pm, o_ld, o_lm, out_total, ws_points, ws_lines, o_ws_points, o_ws_lines, ws_total; };
TailLayout tail_layout(int np0, int np1, int n0, int k0, int n1, int k1) {
  TailLayout L{};
  Carve c;
  L.o_pd = c.take(sz_mul(np0, np1, 4));
  L.o_pm = c.take((int64_t)np0 * 4);
  L.o_ld = c.take(sz_mul(k0, k1, 4));
  L.o_lm = c.take((int64_t)k0 * 4);
  L.out_total = c.o;
  L.ws_points = np0 > 0 && np1 > 0 ? points_layout(np0, np1).total : 0;
  L.ws_lines = k0 > 0 && k1 > 0 ? match_layout(1, (int64_t)n0 * n1, (int64_t)k0 + k1).total : 0;
  Carve w;
  w.take(L.out_total);
  L.o_ws_points = w.take(L.ws_points);
  L.o_ws_lines = w.take(L.ws_lines);
  L.ws_total = sz_add(w.o, 256);
  return L;
}
}  // namespace

extern "C" int64_t linetr_pair_tail_workspace_bytes(int32_t np0, int32_t np1, int32_t n0, int32_t k0, int32_t n1, int32_t k1) {
  return sz_answer(tail_layout(std::max(np0, 0), std::max(np1, 0), std::max(n0, 0), std::max(k0, 0), std::max(n1, 0), std::max(k1, 0)).ws_total);
}

extern "C" int64_t linetr_pair_tail_output_bytes(int32_t np0, int32_t np1, int32_t k0, int32_t k1, int64_t* h_offsets) {
  const TailLayout L = tail_layout(std::max(np0, 0), std::max(np1, 0), 0, std::max(k0, 0), 0, std::max(k1, 0));
  const bool served = sz_answer(L.out_total) == L.out_total;      // a block beyond any size: 0, and the offsets with it
  if (h_offsets) { h_offsets[0] = served ? L.o_pd : 0; h_offsets[1] = served ? L.o_pm : 0; h_offsets[2] = served ? L.o_ld : 0; h_offsets[3] = served ? L.o_lm : 0; }
  return sz_answer(L.out_total);
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
  char* wsp = dout + L.o_ws_points;
  char* wsl = dout + L.o_ws_lines;
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

namespace {
// workspace of linetr_match_distmat: 256 bytes nobody reads (the pair table travels inline) | identity maps | Dk copy | argmin ints
struct DistmatLayout { int64_t o_id0, o_id1, o_dk, o_scr, total; };
DistmatLayout distmat_layout(int n0, int n1) {
  DistmatLayout L{};
  Carve c;
  c.take(256);
  L.o_id0 = c.take((int64_t)n0 * 4);
  L.o_id1 = c.take((int64_t)std::max(n1, 1) * 4);
  L.o_dk = c.take(sz_mul(n0, std::max(n1, 1), 4));
  L.o_scr = c.take(sz_mul(pair_scratch_ints(n0, n1), 4));
  L.total = c.o;
  return L;
}
}  // namespace

extern "C" int64_t linetr_match_distmat_workspace_bytes(int32_t n0, int32_t n1) {
  return sz_answer(distmat_layout(std::max(n0, 0), std::max(n1, 0)).total);
}

extern "C" int linetr_match_distmat(LinetrHandle* h, const float* d_dist, int32_t n0, int32_t n1, float thr,
                                    int32_t mutual, int32_t* d_match01, void* d_ws, int64_t ws_bytes, void* stream) {
  if (n0 < 0 || n1 < 0) return fail(LINETR_E_ARG, "match_distmat: bad argument");
  if (n0 == 0) return LINETR_OK;
  if (!d_match01 || !d_ws || (n1 > 0 && !d_dist)) return fail(LINETR_E_ARG, "match_distmat: null pointer");
  hipStream_t st = (hipStream_t)stream;
  if (h) LT_HIP(hipSetDevice(h->device));
  const DistmatLayout L = distmat_layout(n0, n1);
  if (!d_ws || ws_bytes < L.total) return fail(LINETR_E_WORKSPACE, "match_distmat: workspace too small (need %lld)", (long long)L.total);
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
  LT_HIP(hipMemcpyAsync(base + L.o_id0, iota, n0 * 4, hipMemcpyHostToDevice, st));
  if (n1 > 0) LT_HIP(hipMemcpyAsync(base + L.o_id1, iota, n1 * 4, hipMemcpyHostToDevice, st));
  if (int e = staging_ring().commit(slot, st)) return e;
  if (n1 > 0)
    if (int e = pool_stage(st, tab, 1, n1, n1, pd->chunks, (const int*)(base + L.o_id0), (const int*)(base + L.o_id1), d_dist,
                           (float*)(base + L.o_dk), (int*)(base + L.o_scr))) return e;
  hipLaunchKernelGGL(pair_final_kernel, dim3(1), dim3(256), 0, st, tab, thr, mutual, d_match01, (int*)(base + L.o_scr));
  LT_LAUNCH_CHECK();
  return LINETR_OK;
}

namespace {
// workspace of linetr_match_distmat_f64: row minima | row argmins | column argmins
struct DistmatF64Layout { int64_t o_row_min, o_row_arg, o_col_arg, total; };
DistmatF64Layout distmat_f64_layout(int n0, int n1) {
  DistmatF64Layout L{};
  Carve c;
  L.o_row_min = c.take((int64_t)n0 * 8);
  L.o_row_arg = c.take((int64_t)n0 * 4);
  L.o_col_arg = c.take((int64_t)std::max(n1, 1) * 4);
  L.total = sz_add(c.o, 256);
  return L;
}
}  // namespace

extern "C" int64_t linetr_match_distmat_f64_workspace_bytes(int32_t n0, int32_t n1) {
  return sz_answer(distmat_f64_layout(std::max(n0, 0), std::max(n1, 0)).total);
}

extern "C" int linetr_match_distmat_f64(LinetrHandle* h, const double* d_dist, int32_t n0, int32_t n1, double thr, int32_t mutual,
                                        int32_t* d_match01, void* d_ws, int64_t ws_bytes, void* stream) {
  if (n0 < 0 || n1 < 0) return fail(LINETR_E_ARG, "match_distmat_f64: bad argument");
  if (n0 == 0) return LINETR_OK;
  if (!d_match01 || !d_ws || (n1 > 0 && !d_dist)) return fail(LINETR_E_ARG, "match_distmat_f64: null pointer");
  const DistmatF64Layout L = distmat_f64_layout(n0, n1);
  if (ws_bytes < L.total) return fail(LINETR_E_WORKSPACE, "match_distmat_f64: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  if (h) LT_HIP(hipSetDevice(h->device));
  if (n1 == 0) { LT_HIP(hipMemsetAsync(d_match01, 0xff, (size_t)n0 * 4, st)); return LINETR_OK; }
  char* base = (char*)d_ws;
  double* row_min = (double*)(base + L.o_row_min);
  int* row_arg = (int*)(base + L.o_row_arg);
  int* col_arg = (int*)(base + L.o_col_arg);
  hipLaunchKernelGGL(argmin_rows_f64_kernel, dim3(cdiv(n0, 4)), dim3(256), 0, st, d_dist, n0, n1, row_arg, row_min);
  hipLaunchKernelGGL(argmin_cols_f64_kernel, dim3(cdiv(n1, 256)), dim3(256), 0, st, d_dist, n0, n1, col_arg);
  hipLaunchKernelGGL(match_final_f64_kernel, dim3(cdiv(n0, 256)), dim3(256), 0, st, (const int*)row_arg, (const double*)row_min,
                     (const int*)col_arg, n0, thr, mutual, d_match01);
  LT_LAUNCH_CHECK();
  return LINETR_OK;
}

// subline2keyline (models/line_transformer.py:277-282) alone: Dk = A0 D A1^T for the segmented-mean matrices the tokeniser
// produces, given as sub-line -> key-line maps (non-decreasing).  Same kernel as linetr_match's pooling stage.
static int64_t pool_distmat_bytes(int k0, int k1) { return sz_add(align_up(sz_mul(pair_scratch_ints(std::max(k0, 0), std::max(k1, 0)), 4), 256), 256); }
extern "C" int64_t linetr_pool_distmat_workspace_bytes(int32_t k0, int32_t k1) { return sz_answer(pool_distmat_bytes(k0, k1)); }

extern "C" int linetr_pool_distmat(LinetrHandle* h, const float* d_dist, int32_t n0, int32_t n1, const int32_t* d_s2l0, int32_t k0,
                                   const int32_t* d_s2l1, int32_t k1, float* d_dk, void* d_ws, int64_t ws_bytes, void* stream) {
  if (n0 < 0 || n1 < 0 || k0 < 0 || k1 < 0 || k0 > n0 || k1 > n1) return fail(LINETR_E_ARG, "pool_distmat: bad dims");
  if (k0 == 0 || k1 == 0) return LINETR_OK;
  if (!d_dist || !d_s2l0 || !d_s2l1 || !d_dk || !d_ws) return fail(LINETR_E_ARG, "pool_distmat: null pointer");
  if (ws_bytes < pool_distmat_bytes(k0, k1)) return fail(LINETR_E_WORKSPACE, "pool_distmat: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  if (h) LT_HIP(hipSetDevice(h->device));
  PairTable tab{};
  tab.n_inline = 1;
  PairDesc* pd = tab.inl;
  pd->n0 = n0; pd->k0 = k0; pd->n1 = n1; pd->k1 = k1;
  pd->chunks = cdiv(k0, PM_ROWS);
  ProfScope ps(h, st, "pair_pool", 0, 4.0 * ((double)n0 * n1 + (double)k0 * k1));
  return pool_stage(st, tab, 1, n1, k1, pd->chunks, d_s2l0, d_s2l1, d_dist, d_dk, (int*)d_ws);
}

// subline2keyline on the two mat_klines2sublines MATRICES, as the reference's call sites hand them over (models/matching.py:80:
// data['mat_klines2sublines0'][0], a [K,N] float32 tensor).  A tokeniser's matrix is reduced to its sub-line -> key-line map on the
// device and pooled by the segmented-mean kernel; any other matrix is multiplied out as given.  Asynchronous on `stream`.
namespace {
struct DensePoolLayout { int64_t o_map0, o_map1, o_val0, o_val1, o_verdict, o_tmp, o_pool, total; };
DensePoolLayout dense_pool_layout(int k0, int n0, int k1, int n1) {
  DensePoolLayout L{};
  Carve c;
  L.o_verdict = c.take(4);                           // FIRST: the header promises the verdict word at the workspace's offset 0
  L.o_map0 = c.take((int64_t)std::max(n0, 1) * 4);
  L.o_map1 = c.take((int64_t)std::max(n1, 1) * 4);
  L.o_val0 = c.take((int64_t)std::max(n0, 1) * 4);
  L.o_val1 = c.take((int64_t)std::max(n1, 1) * 4);
  L.o_tmp = c.take(sz_mul(std::max(k0, 1), std::max(n1, 1), 4));
  L.o_pool = c.take(pool_distmat_bytes(std::min(k0, n0), std::min(k1, n1)));
  L.total = c.o;
  return L;
}
}  // namespace

extern "C" int64_t linetr_pool_distmat_dense_workspace_bytes(int32_t k0, int32_t n0, int32_t k1, int32_t n1) {
  return sz_answer(dense_pool_layout(std::max(k0, 0), std::max(n0, 0), std::max(k1, 0), std::max(n1, 0)).total);
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

namespace {
// a type code of linetr_superpoint_heads_typed -> MapType, or -1
int head_type(int32_t code) { return code == 0 ? MT_F32 : code == LINETR_DENSE_F16 ? MT_F16 : code == LINETR_DENSE_BF16 ? MT_BF16 : -1; }
bool aligned_to(const void* p, int bytes) { return (reinterpret_cast<uintptr_t>(p) & (uintptr_t)(bytes - 1)) == 0; }

// the NCHW descriptor head for raw inputs of type EI: the float32 / float32 pair is the kernel that was always there
template <class EI, class EO>
void desc_head_launch(hipStream_t st, int B, int HW, const void* raw, void* nhwc, void* nchw) {
  const dim3 grid((unsigned)cdiv(HW, 32), (unsigned)B);
  if constexpr (sizeof(EI) == 4 && sizeof(EO) == 4)
    hipLaunchKernelGGL((sp_desc_head_kernel<32, false>), grid, dim3(256), 0, st, (const float*)raw, (float*)nhwc, (float*)nchw, HW, (int64_t)0);
  else
    hipLaunchKernelGGL((sp_desc_head_typed_kernel<32, EI, EO>), grid, dim3(256), 0, st, (const EI*)raw, (EO*)nhwc, (EO*)nchw, HW);
}
template <class EI>
void desc_head_launch_in(hipStream_t st, int out_type, int B, int HW, const void* raw, void* nhwc, void* nchw) {
  if (out_type == MT_F32) desc_head_launch<EI, float>(st, B, HW, raw, nhwc, nchw);
  else if (out_type == MT_F16) desc_head_launch<EI, f16_t>(st, B, HW, raw, nhwc, nchw);
  else desc_head_launch<EI, bf16_t>(st, B, HW, raw, nhwc, nchw);
}

// Both layouts of the raw head outputs: NCHW (rows = false; the strides are unused) or channel-last rows of ld_score / ld_desc floats.
// in_type / out_type (MapType): the element type of the two raw inputs and of the two descriptor outputs; rows are float32 only.
template <bool ROWS>
int superpoint_heads_any(LinetrHandle* h, const char* who, const void* d_score, int64_t ld_score, const void* d_desc, int64_t ld_desc,
                         int in_type, int32_t B, int32_t Hc, int32_t Wc, float* d_dense_score, void* d_dense_desc_nhwc,
                         void* d_dense_desc_nchw, int out_type, void* stream) {
  if (in_type < 0 || out_type < 0 || (ROWS && (in_type != MT_F32 || out_type != MT_F32)))
    return fail(LINETR_E_ARG, "%s: a type code must be 0 (float32), LINETR_DENSE_F16 or LINETR_DENSE_BF16", who);
  if (B < 0 || Hc <= 0 || Wc <= 0) return fail(LINETR_E_ARG, "%s: bad shape B=%d Hc=%d Wc=%d", who, B, Hc, Wc);
  if (d_dense_score && !d_score) return fail(LINETR_E_ARG, "%s: score output without score logits", who);
  if ((d_dense_desc_nhwc || d_dense_desc_nchw) && !d_desc) return fail(LINETR_E_ARG, "%s: descriptor output without the raw descriptor head", who);
  if (ROWS && ((d_score && ld_score < 65) || (d_desc && ld_desc < D))) return fail(LINETR_E_ARG, "%s: row stride below the row's length", who);
  // 16-byte vectors: every output (the score map and the NCHW map are stored so, the channel-last map is what the samplers load so) and
  // the NCHW head outputs when a channel's plane is a multiple of 4 floats; rows are read scalar-wise.  A half side moves 4 elements as
  // 8 bytes; off the vector path a half input needs its own 2.
  const bool vec_in = !ROWS && ((int64_t)Hc * Wc) % 4 == 0;
  const int in_align = in_type == MT_F32 ? (vec_in ? 16 : 1) : (vec_in ? 8 : 2), out_align = out_type == MT_F32 ? 16 : 8;
  if (!aligned16(d_dense_score) || !aligned_to(d_dense_desc_nhwc, out_align) || !aligned_to(d_dense_desc_nchw, out_align) ||
      !aligned_to(d_score, in_align) || !aligned_to(d_desc, in_align))
    return fail(LINETR_E_ARG, "%s: the dense maps%s must be 16-byte aligned (half descriptor maps and half inputs: 8)", who,
                vec_in ? " and the raw head outputs" : "");
  if (B == 0) return LINETR_OK;
  if (h) LT_HIP(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  const int HW = Hc * Wc;
  const dim3 grid((unsigned)cdiv(HW, 64), (unsigned)B);
  const double in_b = in_type == MT_F32 ? 4.0 : 2.0, out_b = out_type == MT_F32 ? 4.0 : 2.0;
  if (d_dense_desc_nhwc || d_dense_desc_nchw) {
    const double by = (double)B * HW * D * (in_b + out_b * ((d_dense_desc_nhwc ? 1 : 0) + (d_dense_desc_nchw ? 1 : 0)));
    ProfScope ps(h, st, "sp_desc_head", 3.0 * B * HW * D, by);
    if constexpr (ROWS)
      hipLaunchKernelGGL((sp_desc_head_kernel<32, true>), dim3((unsigned)cdiv(HW, 32), (unsigned)B), dim3(256), 0, st, (const float*)d_desc,
                         (float*)d_dense_desc_nhwc, (float*)d_dense_desc_nchw, HW, ld_desc);
    else if (in_type == MT_F32) desc_head_launch_in<float>(st, out_type, B, HW, d_desc, d_dense_desc_nhwc, d_dense_desc_nchw);
    else if (in_type == MT_F16) desc_head_launch_in<f16_t>(st, out_type, B, HW, d_desc, d_dense_desc_nhwc, d_dense_desc_nchw);
    else desc_head_launch_in<bf16_t>(st, out_type, B, HW, d_desc, d_dense_desc_nhwc, d_dense_desc_nchw);
    LT_LAUNCH_CHECK();
  }
  if (d_dense_score) {
    ProfScope ps(h, st, "sp_score_head", 0, (double)B * HW * (65 * in_b + 64 * 4.0));
    if (in_type == MT_F32) hipLaunchKernelGGL(sp_score_head_kernel<ROWS>, grid, dim3(256), 0, st, (const float*)d_score, d_dense_score, Hc, Wc, ld_score);
    else if (in_type == MT_F16) hipLaunchKernelGGL(sp_score_head_typed_kernel<f16_t>, grid, dim3(256), 0, st, (const f16_t*)d_score, d_dense_score, Hc, Wc);
    else hipLaunchKernelGGL(sp_score_head_typed_kernel<bf16_t>, grid, dim3(256), 0, st, (const bf16_t*)d_score, d_dense_score, Hc, Wc);
    LT_LAUNCH_CHECK();
  }
  return LINETR_OK;
}
}  // namespace

extern "C" int linetr_superpoint_heads(LinetrHandle* h, const float* d_score_logits, const float* d_desc_raw, int32_t B,
                                       int32_t Hc, int32_t Wc, float* d_dense_score, float* d_dense_desc_nhwc,
                                       float* d_dense_desc_nchw, void* stream) {
  return superpoint_heads_any<false>(h, "superpoint_heads", d_score_logits, 0, d_desc_raw, 0, MT_F32, B, Hc, Wc, d_dense_score,
                                     d_dense_desc_nhwc, d_dense_desc_nchw, MT_F32, stream);
}

extern "C" int linetr_superpoint_heads_typed(LinetrHandle* h, const void* d_score_logits, const void* d_desc_raw, int32_t in_type, int32_t B,
                                             int32_t Hc, int32_t Wc, float* d_dense_score, void* d_dense_desc_nhwc,
                                             void* d_dense_desc_nchw, int32_t out_type, void* stream) {
  return superpoint_heads_any<false>(h, "superpoint_heads_typed", d_score_logits, 0, d_desc_raw, 0, head_type(in_type), B, Hc, Wc,
                                     d_dense_score, d_dense_desc_nhwc, d_dense_desc_nchw, head_type(out_type), stream);
}

extern "C" int linetr_superpoint_heads_rows(LinetrHandle* h, const float* d_score_rows, int64_t ld_score, const float* d_desc_rows,
                                            int64_t ld_desc, int32_t B, int32_t Hc, int32_t Wc, float* d_dense_score,
                                            float* d_dense_desc_nhwc, float* d_dense_desc_nchw, void* stream) {
  return superpoint_heads_any<true>(h, "superpoint_heads_rows", d_score_rows, ld_score, d_desc_rows, ld_desc, MT_F32, B, Hc, Wc, d_dense_score,
                                    d_dense_desc_nhwc, d_dense_desc_nchw, MT_F32, stream);
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
  Carve c;
  L.o_mask = c.take(sz_mul(B, H, L.Wm, 4));
  L.o_rowoff = c.take(sz_mul(B, H, 4));
  L.o_keys = c.take(sz_mul(B, cap, 8));
  L.total = sz_add(c.o, 256);
  return L;
}

// sp_nms_kernel takes more than 64 KiB of dynamic LDS: raised once per device
bool kp_lds_ok() { return allow_dynamic_lds<sp_nms_kernel>((int)kp_nms_lds(KP_MAX_R)) == hipSuccess; }
}  // namespace

extern "C" int64_t linetr_superpoint_keypoints_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t cap_per_image) {
  if ((int64_t)std::max(H, 0) * std::max(W, 0) > INT32_MAX || (int64_t)std::max(B, 0) * std::max(H, 0) > INT32_MAX) return 0;   // refused by the entry point
  return sz_answer(kp_layout(std::max(B, 0), std::max(H, 0), std::max(W, 0), std::max(cap_per_image, 0)).total);
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
