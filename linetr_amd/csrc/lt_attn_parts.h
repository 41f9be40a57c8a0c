// The pieces the signature-attention kernels share (lt_attn.h, lt_attn_fused.h, experiments/csrc): device helpers only, no
// __global__ function, so that every translation unit may include it.  A piece is used wherever the kernel's instructions stay
// exactly as they were with the text written out (tools/kernel_isa_diff.py; profiles/attn_refactor_isa.txt lists the sites).
#pragma once
#include "lt_gemm_split.h"

namespace lt {

// 8 fp32 -> the three bf16 planes of one MFMA operand fragment (8 consecutive k of a lane)
__device__ __forceinline__ void split8(float x0, float x1, float x2, float x3, float x4, float x5, float x6, float x7, bf16x8 (&o)[3]) {
  unsigned a[3], b[3], c[3], d[3];
  split_pair<3>(x0, x1, a); split_pair<3>(x2, x3, b);
  split_pair<3>(x4, x5, c); split_pair<3>(x6, x7, d);
#pragma unroll
  for (int p = 0; p < 3; ++p) {
    union { bf16x8 v; unsigned w[4]; } u;
    u.w[0] = a[p]; u.w[1] = b[p]; u.w[2] = c[p]; u.w[3] = d[p];
    o[p] = u.v;
  }
}
__device__ __forceinline__ void split8(const f32x4& x0, const f32x4& x1, bf16x8 (&o)[3]) {
  split8(x0[0], x0[1], x0[2], x0[3], x1[0], x1[1], x1[2], x1[3], o);
}
// P^T planes of the 16-wide kv step t straight from the S^T accumulator: its k-slot e is register 8 t + e
__device__ __forceinline__ void split_p(const f32x16& st, int t, bf16x8 (&o)[3]) {
  split8(st[8 * t], st[8 * t + 1], st[8 * t + 2], st[8 * t + 3], st[8 * t + 4], st[8 * t + 5], st[8 * t + 6], st[8 * t + 7], o);
}

// acc += a . b on three planes: the six products in split_terms<3> order, smallest first
__device__ __forceinline__ void mma6(const bf16x8 (&a)[3], const bf16x8 (&b)[3], f32x16& acc) {
#pragma unroll
  for (int t = 0; t < split_terms<3>::N; ++t) acc = mfma_split<0>(a[split_terms<3>::pa(t)], b[split_terms<3>::pb(t)], acc);
}

// Q fragments of a lane (B operand of S^T = K Q^T): channels 16 s + 8 h2 .. + 8 of its query row, qp = row + 8 h2, times
// LOG2E -- scores in log2 units: exp -> v_exp_f32 -- and split
__device__ __forceinline__ void q_frags(const float* qp, bf16x8 (&qf)[4][3]) {
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    f32x4 x0 = *reinterpret_cast<const f32x4*>(qp + s * 16);
    f32x4 x1 = *reinterpret_cast<const f32x4*>(qp + s * 16 + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) { x0[e] *= LOG2E; x1[e] *= LOG2E; }
    split8(x0, x1, qf[s]);
  }
}

// Six transposing LDS reads (gfx950 ds_read_b64_tr_b16) = the V^T fragments of one 16-wide kv step and one 32-wide d block
// from a ROW-major V image: the hardware hands lane (d = lane & 31, half h) the four values V[kv + 4 h + j][d], j = 0..3 --
// exactly the k-slots the P^T accumulator registers occupy (tools/ubench/tr_read_probe.hip prints the mapping).  Within a
// 16-lane group lane i addresses row (i >> 2), 4-column chunk (i & 3); lanes 16-31 take the next 16 columns, the upper
// half-wave starts 4 rows down.  R0 / R1 = byte offsets of the two kv runs (8 rows apart) from the lane's `base`, PB = bytes
// between planes.  o[p][0/1]: plane p, run R0 / R1.  WAIT = false leaves the reads in flight: hipcc does not count an asm load,
// so the consumer then calls tr_wait, one lgkmcnt(0) that names every destination (cdna_hip_programming.md 5.7).
__device__ __forceinline__ void tr_wait(u32x2 (&o)[3][2]) {
  asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(o[0][0]), "+v"(o[0][1]), "+v"(o[1][0]), "+v"(o[1][1]), "+v"(o[2][0]), "+v"(o[2][1]) : : "memory");
}
// (a macro only because the text of an asm statement cannot be a template parameter: the flag picks one of two statements)
#define LT_TR_READS6(tail)                                                                                           \
  asm volatile("ds_read_b64_tr_b16 %0, %6 offset:%7\n\t"                                                            \
               "ds_read_b64_tr_b16 %1, %6 offset:%8\n\t"                                                            \
               "ds_read_b64_tr_b16 %2, %6 offset:%9\n\t"                                                            \
               "ds_read_b64_tr_b16 %3, %6 offset:%10\n\t"                                                           \
               "ds_read_b64_tr_b16 %4, %6 offset:%11\n\t"                                                           \
               "ds_read_b64_tr_b16 %5, %6 offset:%12" tail                                                          \
               : "=&v"(o[0][0]), "=&v"(o[0][1]), "=&v"(o[1][0]), "=&v"(o[1][1]), "=&v"(o[2][0]), "=&v"(o[2][1])     \
               : "v"(base), "n"(R0), "n"(R1), "n"(R0 + PB), "n"(R1 + PB), "n"(R0 + 2 * PB), "n"(R1 + 2 * PB)        \
               : "memory")
template <int R0, int R1, int PB, bool WAIT>
__device__ __forceinline__ void tr_reads(unsigned base, u32x2 (&o)[3][2]) {
  if constexpr (WAIT) LT_TR_READS6("\n\ts_waitcnt lgkmcnt(0)");    // (inside the statement: a tr_wait behind it moves the callers' instructions)
  else LT_TR_READS6("");
}
#undef LT_TR_READS6

}  // namespace lt
