// The pieces the signature-attention kernels share (lt_attn.h, lt_attn_fused.h, lt_attnbwd.h, experiments/csrc): device helpers
// only, no __global__ function, so that every translation unit may include it.  The split-bf16 pieces are used wherever the kernel's
// instructions stay exactly as they were with the text written out (tools/kernel_isa_diff.py; profiles/attn_refactor_isa.txt lists
// the sites); sig_attn_tile, the whole body of the two exact-fp32 forward kernels, moved a few of their instructions and was gated on
// output bits instead (tools/entry_point_digest.py; profiles/train_fwd_once_isa.txt, train_fwd_once_digest.txt).
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

// ---------------------------------------------------------------------------------------------
// The exact-fp32 attention tile: 128 queries of one head of one image against all of the image's keys.  Flash-style, fp32 MFMA
// (v_mfma_f32_32x32x2_f32), natural-log scores and expf, no n x n matrix in memory.  The body of sig_attn_kernel (lt_attn.h,
// TRAIN = false: q arrives pre-scaled by 1/8, lse is not touched) and of ab_fwd_kernel (lt_attnbwd.h, TRAIN = true: q is multiplied
// by 1/8 on load -- a power of two, exact -- and lse = m + logf(l) is stored per (row, head)).  The summation order of the message
// lives here and nowhere else, so the two kernels' messages have the same bits.
//
// block 256 = 4 wave64, wave w owns 32 query rows.  Q, K, V, out: row 0 of the BATCH, column 0 of head 0, a row stride each (they
// may be column blocks of one buffer; all are only read).  n0, Ni: the image's first row and row count; q0 < Ni: the tile's first
// query within the image.  Per 32-row kv chunk and wave:
//   S^T[kv][q] = K_h[kv,:] . Q_h[q,:]      (A = K tile from LDS, B = Q fragment held in VGPRs)
//   in the 32x32 C/D layout a lane owns ONE query column (q = lane&31) and 16 kv rows, so the online
//   softmax max/sum are in-lane + one exchange with lane^32;
//   the exponentiated S^T registers ARE the B operand of  O^T[d][q] += V^T[d][kv] . P^T[kv][q]
//   under the k-permutation k = 8kk + 4*(lane>>5) + s  <->  register 4kk+s, so P never leaves VGPRs.
// Keys beyond the image are staged as zeros and score -inf; nothing beyond the image is loaded or stored.
// ---------------------------------------------------------------------------------------------
constexpr int ATT_QT = 128;      // rows a block owns (4 waves x 32): queries here and in ab_dq, keys in ab_dkv
constexpr int ATT_KT = 64;       // rows of the other side staged per iteration
constexpr int ATT_KS = DH + 4;   // padded LDS row stride

template <bool TRAIN>
__device__ __forceinline__ void sig_attn_tile(const float* __restrict__ Q, int64_t ldq, const float* __restrict__ K, int64_t ldk,
                                              const float* __restrict__ V, int64_t ldv, int n0, int Ni, int q0, int head,
                                              float* __restrict__ out, int64_t ldo, float* __restrict__ lse /*[N][4], TRAIN only*/) {
  __shared__ __attribute__((aligned(16))) float Ks[ATT_KT * ATT_KS];
  __shared__ __attribute__((aligned(16))) float Vs[ATT_KT * DH];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h2 = lane >> 5, lq = lane & 31;
  const int q = q0 + wave * 32 + lq;
  const bool wave_active = q0 + wave * 32 < Ni;  // wave-uniform
  const float* kbase = K + (int64_t)n0 * ldk + head * DH;
  const float* vbase = V + (int64_t)n0 * ldv + head * DH;

  f32x4 qf[8];
  {
    const int qr = q < Ni ? q : Ni - 1;   // a lane behind the image repeats its last query; it stores nothing
    const float* qp = Q + (int64_t)(n0 + qr) * ldq + head * DH + h2 * 4;
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) {
      qf[kk] = *reinterpret_cast<const f32x4*>(qp + kk * 8);
      if constexpr (TRAIN) {
#pragma unroll
        for (int e = 0; e < 4; ++e) qf[kk][e] *= 0.125f;
      }
    }
  }
  f32x16 o0, o1;
#pragma unroll
  for (int r = 0; r < 16; ++r) { o0[r] = 0.f; o1[r] = 0.f; }
  float m = -INFINITY, l = 0.f;

  const int srow = tid >> 4, sc4 = (tid & 15) * 4;  // staging: 16 rows x 16 float4 per pass
  for (int t0 = 0; t0 < Ni; t0 += ATT_KT) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = srow + i * 16;
      const int kv = t0 + r;
      f32x4 kx = {0.f, 0.f, 0.f, 0.f}, vx = {0.f, 0.f, 0.f, 0.f};
      if (kv < Ni) {
        kx = *reinterpret_cast<const f32x4*>(kbase + (int64_t)kv * ldk + sc4);
        vx = *reinterpret_cast<const f32x4*>(vbase + (int64_t)kv * ldv + sc4);
      }
      *reinterpret_cast<f32x4*>(&Ks[r * ATT_KS + sc4]) = kx;
      *reinterpret_cast<f32x4*>(&Vs[r * DH + sc4]) = vx;
    }
    __syncthreads();
    if (!wave_active) continue;
#pragma unroll
    for (int c = 0; c < ATT_KT / 32; ++c) {
      const int kv0 = t0 + c * 32;
      if (kv0 >= Ni) break;
      f32x16 st;
#pragma unroll
      for (int r = 0; r < 16; ++r) st[r] = 0.f;
      const float* kp = &Ks[(c * 32 + lq) * ATT_KS + h2 * 4];
#pragma unroll
      for (int kk = 0; kk < 8; ++kk) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(kp + kk * 8);
#pragma unroll
        for (int s = 0; s < 4; ++s) st = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], qf[kk][s], st, 0, 0, 0);
      }
      // online softmax over this lane's 16 kv rows (+ the other half-wave's 16)
      if (kv0 + 32 > Ni) {   // wave-uniform: only the image's last chunk has keys past the end
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (kv0 + (r & 3) + 8 * (r >> 2) + 4 * h2 >= Ni) st[r] = -INFINITY;
      }
      float mx = st[0];
#pragma unroll
      for (int r = 1; r < 16; ++r) mx = fmaxf(mx, st[r]);
      mx = xor32_max(mx);
      const float m_new = fmaxf(m, mx);
      const float alpha = expf(m - m_new);  // m = -inf on the first chunk -> 0  (natural-log scores and expf: the exact-fp32 reference path)
      float ps = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) { st[r] = expf(st[r] - m_new); ps += st[r]; }
      ps = xor32_sum(ps);
      l = l * alpha + ps;
      m = m_new;
#pragma unroll
      for (int r = 0; r < 16; ++r) { o0[r] *= alpha; o1[r] *= alpha; }
      // O^T += V^T . P^T
      const float* vp = &Vs[(c * 32 + h2 * 4) * DH + lq];
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const float v0 = vp[(kk * 8 + s) * DH];
          const float v1 = vp[(kk * 8 + s) * DH + 32];
          o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(v0, st[kk * 4 + s], o0, 0, 0, 0);
          o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(v1, st[kk * 4 + s], o1, 0, 0, 0);
        }
      }
    }
  }
  if (wave_active && q < Ni) {
    const float inv = 1.f / l;
    float* op = out + (int64_t)(n0 + q) * ldo + head * DH;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int d = (r & 3) + 8 * (r >> 2) + 4 * h2;
      op[d] = o0[r] * inv;
      op[d + 32] = o1[r] * inv;
    }
    if constexpr (TRAIN) {
      if (h2 == 0) lse[(int64_t)(n0 + q) * HEADS + head] = m + logf(l);   // (both halves hold the same m and l)
    }
  }
}

}  // namespace lt
