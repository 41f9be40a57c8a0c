// Common definitions for the gfx950 LineTR library (host + device).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/linetr_hip.h"

namespace lt {

constexpr int D = 256;      // descriptor_dim
constexpr int HEADS = 4;
constexpr int DH = 64;      // D / HEADS
constexpr int POOLW = 544;  // pooled row per head: [dbar(256) | abar(256) | p0 | 31 zeros]
constexpr int WAVE = 64;
// widest BatchNorm layer the statistics scratch of linetr_forward_train is sized for (2 D of the signature MLPs at D = 256, lt_bntrain.h);
// the weight preparation (lt_prepare.h) refuses a training-mode handle with a wider layer
constexpr int BN_MAX_CHANNELS = 512;

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// Element types of a dense descriptor map or a raw head output (LINETR_DENSE_F16 / LINETR_DENSE_BF16, include/linetr_hip.h).  Arithmetic
// is float32 throughout: Elem<E>::widen is exact (fp16 subnormals included), Elem<E>::narrow rounds to nearest-even as torch's
// .half() / .bfloat16() do.  raw4 is what a lane holds of its 4 channels between the load and the first use: 16 bytes of float32, 8 of a
// half type.
typedef _Float16 f16_t;
struct bf16_t { uint16_t bits; };
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef uint16_t u16x4 __attribute__((ext_vector_type(4)));
enum MapType { MT_F32 = 0, MT_F16 = 1, MT_BF16 = 2 };

template <class E> struct Elem;
template <> struct Elem<float> {
  typedef f32x4 raw4;
  static __device__ __forceinline__ f32x4 widen(f32x4 v) { return v; }
  static __device__ __forceinline__ float widen(float v) { return v; }
  static __device__ __forceinline__ float narrow(float v) { return v; }
};
template <> struct Elem<f16_t> {
  typedef f16x4 raw4;
  static __device__ __forceinline__ f32x4 widen(f16x4 v) { return __builtin_convertvector(v, f32x4); }
  static __device__ __forceinline__ float widen(f16_t v) { return (float)v; }
  static __device__ __forceinline__ f16_t narrow(float v) { return (f16_t)v; }
};
template <> struct Elem<bf16_t> {
  typedef u16x4 raw4;
  static __device__ __forceinline__ float widen(bf16_t v) { return __builtin_bit_cast(float, (uint32_t)v.bits << 16); }
  static __device__ __forceinline__ f32x4 widen(u16x4 v) {
    return f32x4{widen(bf16_t{v[0]}), widen(bf16_t{v[1]}), widen(bf16_t{v[2]}), widen(bf16_t{v[3]})};
  }
  static __device__ __forceinline__ bf16_t narrow(float v) {
    const uint32_t u = __builtin_bit_cast(uint32_t, v);
    if ((u & 0x7fffffffu) > 0x7f800000u) return bf16_t{0x7fc0};            // NaN (torch's quiet NaN)
    return bf16_t{(uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16)};    // round to nearest, ties to even
  }
};
// this lane's 4 consecutive elements, `p` on the 4-element grid (16 bytes of float32, 8 of a half type): one load
template <class E>
__device__ __forceinline__ typename Elem<E>::raw4 load_raw4(const E* p) {
  return *reinterpret_cast<const typename Elem<E>::raw4*>(p);
}

// The shipped library (liblinetr_hip.so) is built WITHOUT LINETR_EXPERIMENTS: no tuning switches, none of the kernels that
// were measured and lost.  `python -m linetr_amd.build --experiments` builds liblinetr_hip_experiments.so from the same sources
// plus experiments/csrc: the stream-K tail, the 256x256 tile, the fused signature MLP, the split-tile / LDS-DMA path, the
// row-owner GEMM, GEMM chains and the single-pair persistent network, and the switches that select them or that tools/ and
// experiments/test_experiments.py read.  Apart from the 256x256 case of gemm_split_launch (lt_gemm_split.h), those kernels and
// their host code live in experiments/csrc and reach the forward pass through a few one-line hooks in linetr_net.hip
// (experiments/csrc/lt_x_net.h).  LT_XENV is getenv there and a constant null pointer in the product, so every switch on a
// shipped path folds away.
#ifdef LINETR_EXPERIMENTS
#define LT_XENV(name) getenv(name)
#else
#define LT_XENV(name) (static_cast<const char*>(nullptr))
#endif

inline thread_local std::string g_err;

inline int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

#define LT_HIP(expr)                                                                        \
  do {                                                                                      \
    hipError_t e_ = (expr);                                                                 \
    if (e_ != hipSuccess)                                                                   \
      return lt::fail(LINETR_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_),  \
                      __FILE__, __LINE__);                                                  \
  } while (0)

#define LT_LAUNCH_CHECK()                                                                   \
  do {                                                                                      \
    hipError_t e_ = hipGetLastError();                                                      \
    if (e_ != hipSuccess)                                                                   \
      return lt::fail(LINETR_E_HIP, "kernel launch failed: %s (%s:%d)", hipGetErrorString(e_), \
                      __FILE__, __LINE__);                                                  \
  } while (0)

// Sizes.  Every byte count a size query or a layout function forms goes through sz_mul / sz_add / align_up / Carve: non-negative
// int64_t arithmetic that SATURATES at SZ_LIMIT instead of leaving its type (a negative operand saturates too).  No workspace is
// anywhere near 2^56 bytes, so a saturated total means "a shape no entry point serves": a query returns sz_answer(total) = 0 for it and
// never a wrapped number, and an entry point's `workspace_bytes < total` refuses it.  Below the limit every value is what plain
// arithmetic gives.
constexpr int64_t SZ_LIMIT = int64_t(1) << 56;
inline int64_t sz_mul(int64_t a, int64_t b) {
  int64_t r;
  return (a < 0 || b < 0 || __builtin_mul_overflow(a, b, &r) || r > SZ_LIMIT) ? SZ_LIMIT : r;
}
template <class... T> inline int64_t sz_mul(int64_t a, int64_t b, T... more) { return sz_mul(sz_mul(a, b), more...); }
inline int64_t sz_add(int64_t a, int64_t b) {
  int64_t r;
  return (a < 0 || b < 0 || __builtin_add_overflow(a, b, &r) || r > SZ_LIMIT) ? SZ_LIMIT : r;
}
template <class... T> inline int64_t sz_add(int64_t a, int64_t b, T... more) { return sz_add(sz_add(a, b), more...); }
inline int64_t sz_answer(int64_t total) { return total >= SZ_LIMIT || total < 0 ? 0 : total; }
inline int64_t align_up(int64_t v, int64_t a) { return (v < 0 || v > SZ_LIMIT - a) ? SZ_LIMIT : (v + a - 1) / a * a; }
// What every entry point asks of a pointer its kernels access with 16-byte vectors (NULL passes: an absent optional pointer).
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
// An entry point's `dense_is_nhwc` argument taken apart (LINETR_DENSE_F16 / LINETR_DENSE_BF16, include/linetr_hip.h): layout, element
// type, element size, and the alignment the kernels need of the caller's map (float32 NHWC 16 bytes and a float32 NCHW map anywhere, as
// ever; a half NHWC map 8, a lane's 4 channels; a half NCHW map its element's 2, the layout pass chooses its vector path row by row).
// Every value below 0x100 means what it always meant, the negative ones included: non-zero = NHWC float32.
struct MapFormat {
  bool nhwc = false; int type = MT_F32; int esize = 4;
  bool aligned(const void* p) const {
    const int need = nhwc ? 4 * esize : type == MT_F32 ? 1 : esize;
    return (reinterpret_cast<uintptr_t>(p) & (uintptr_t)(need - 1)) == 0;
  }
};
inline bool map_format_ok(int dense_is_nhwc, MapFormat& f) {
  if (dense_is_nhwc < 0) { f = MapFormat{}; f.nhwc = true; return true; }
  const int t = dense_is_nhwc & (LINETR_DENSE_F16 | LINETR_DENSE_BF16);
  if ((dense_is_nhwc & ~0x3ff) || t == (LINETR_DENSE_F16 | LINETR_DENSE_BF16)) return false;
  f.nhwc = (dense_is_nhwc & 0xff) != 0;
  f.type = t == LINETR_DENSE_F16 ? MT_F16 : t == LINETR_DENSE_BF16 ? MT_BF16 : MT_F32;
  f.esize = t ? 2 : 4;
  return true;
}
inline int map_format(int dense_is_nhwc, const char* who, MapFormat& f) {
  if (map_format_ok(dense_is_nhwc, f)) return 0;
  return fail(LINETR_E_ARG, "%s: dense_is_nhwc = 0x%x: at most one of LINETR_DENSE_F16 / LINETR_DENSE_BF16 and no higher bit", who,
              (unsigned)dense_is_nhwc);
}
// A workspace carved into 256-byte aligned segments: take(bytes) is the next segment's offset, `o` what has been handed out so far.
struct Carve {
  int64_t o = 0;
  int64_t take(int64_t bytes) { const int64_t at = o; o = sz_add(o, align_up(bytes, 256)); return at; }
};
// A launch with more dynamic LDS than the default limit needs the kernel opted in first, on every device it runs on.  Makes that
// call once per kernel and device (one flag word per kernel, one bit per device) and is safe from several host threads: a thread
// sees a device's bit only after the attribute is set there; two first callers at most repeat the same call.  A refusal is returned,
// cleared from HIP's last-error slot and tried again by the next call.
template <auto Kernel>
inline hipError_t allow_dynamic_lds(int bytes) {
  static std::atomic<unsigned long long> done{0};
  int dev = 0;
  (void)hipGetDevice(&dev);
  const unsigned long long dev_bit = 1ull << (dev & 63);
  if (done.load(std::memory_order_acquire) & dev_bit) return hipSuccess;
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e == hipSuccess) done.fetch_or(dev_bit, std::memory_order_release);
  else (void)hipGetLastError();
  return e;
}
inline int cdiv(int a, int b) { return (int)(((int64_t)a + b - 1) / b); }   // the sum in int64_t: a may be INT32_MAX
// Compute units of the device that is current at the first call (256 if it cannot be asked), cached for the process: what
// the persistent launchers size their grids by.
inline int cu_count() {
  static const int n_cu = [] {
    int dev = 0;
    hipDeviceProp_t prop;
    return (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) ? prop.multiProcessorCount : 256;
  }();
  return n_cu;
}

// Philox4x32-10 (Salmon et al., SC'11), the standard multipliers and key increments.  Host and device: the dropout masks of
// lt_dropout.h draw from it in their kernels, the pseudo lines of linetr_make_pseudo_lines on the host.
__host__ __device__ __forceinline__ uint32_t philox_mulhi(uint32_t a, uint32_t b) {
#ifdef __HIP_DEVICE_COMPILE__
  return __umulhi(a, b);
#else
  return (uint32_t)(((uint64_t)a * (uint64_t)b) >> 32);
#endif
}
__host__ __device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t (&w)[4]) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint32_t hi0 = philox_mulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = philox_mulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}

// ---- device helpers -------------------------------------------------------------------------

// constants of the CLS-row attention pooling (lt_model.h: the cls_pool kernels; prepared in float64 by lt_prepare.h)
struct ClsPoolConst {
  const float* U;     // [4][256]  u_h
  const float* U2;    // [4][256]  W5^T u_h
  float c_tok[4];     // u_h.b5 + c_h   (additive constant of token rows)
  float s_cls[4];     // u_h.cls + c_h  (score of the CLS key, row 0)
};

constexpr float LOG2E = 1.44269504088896340736f;

// Wave-wide reductions on the VALU's DPP paths (no LDS crossbar): xor-1 / xor-2 inside quads, half-row and row
// mirrors give every lane its 16-lane row total, row_bcast15 / row_bcast31 fold the four rows into row 3, and lane 63 is
// broadcast through an SGPR.  7 dependent VALU steps instead of 6 dependent ds_bpermute round trips (__shfl_xor).
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_get(float v, float masked) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, masked), __builtin_bit_cast(int, v),
                                                               CTRL, ROW_MASK, 0xf, false));
}
__device__ __forceinline__ float wave_sum(float v) {
  v += dpp_get<0xB1, 0xf>(v, 0.f);    // quad_perm [1,0,3,2]
  v += dpp_get<0x4E, 0xf>(v, 0.f);    // quad_perm [2,3,0,1]
  v += dpp_get<0x141, 0xf>(v, 0.f);   // row_half_mirror
  v += dpp_get<0x140, 0xf>(v, 0.f);   // row_mirror
  v += dpp_get<0x142, 0xa>(v, 0.f);   // row_bcast15 into rows 1, 3
  v += dpp_get<0x143, 0xc>(v, 0.f);   // row_bcast31 into rows 2, 3
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}
// Exchange between the two 32-lane halves of a wave on gfx950's v_permlane32_swap (no LDS round trip): after the swap one
// register holds the lower half's values in both halves and the other the upper half's, so max / sum of the pair is
// the xor-32 butterfly step, identical in both halves.
// (Inline asm on purpose: with this toolchain __builtin_amdgcn_permlane32_swap hands back the same register for both
// results -- tools/ubench/permlane_test.hip.  The s_nops cover the VALU-write -> permlane-read wait states the
// compiler would otherwise insert itself.)
__device__ __forceinline__ void halves_of(float x, float& lo, float& hi) {
  unsigned a = __builtin_bit_cast(unsigned, x), b = a;
  asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 1" : "+v"(a), "+v"(b));
  lo = __builtin_bit_cast(float, a);
  hi = __builtin_bit_cast(float, b);
}
// a's upper half <-> b's lower half (raw v_permlane32_swap on two different registers)
__device__ __forceinline__ void halves_swap(float& a, float& b) {
  unsigned x = __builtin_bit_cast(unsigned, a), y = __builtin_bit_cast(unsigned, b);
  asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 1" : "+v"(x), "+v"(y));
  a = __builtin_bit_cast(float, x);
  b = __builtin_bit_cast(float, y);
}
__device__ __forceinline__ float xor32_max(float x) { float a, b; halves_of(x, a, b); return fmaxf(a, b); }
__device__ __forceinline__ float xor32_sum(float x) { float a, b; halves_of(x, a, b); return a + b; }

// N independent sums at once: the N chains interleave, so the 2 wait states a DPP read needs after the VALU write of
// its source are filled with useful work instead of s_nops.
template <int N>
__device__ __forceinline__ void wave_sum_n(float (&v)[N]) {
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] += dpp_get<0xB1, 0xf>(v[i], 0.f);
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] += dpp_get<0x4E, 0xf>(v[i], 0.f);
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] += dpp_get<0x141, 0xf>(v[i], 0.f);
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] += dpp_get<0x140, 0xf>(v[i], 0.f);
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] += dpp_get<0x142, 0xa>(v[i], 0.f);
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] += dpp_get<0x143, 0xc>(v[i], 0.f);
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v[i]), 63));
}
__device__ __forceinline__ float wave_max(float v) {
  v = fmaxf(v, dpp_get<0xB1, 0xf>(v, v));
  v = fmaxf(v, dpp_get<0x4E, 0xf>(v, v));
  v = fmaxf(v, dpp_get<0x141, 0xf>(v, v));
  v = fmaxf(v, dpp_get<0x140, 0xf>(v, v));
  v = fmaxf(v, dpp_get<0x142, 0xa>(v, v));
  v = fmaxf(v, dpp_get<0x143, 0xc>(v, v));
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}

}  // namespace lt
