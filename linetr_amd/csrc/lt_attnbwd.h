// Neighbour-line ("signature") attention for training (models/line_transformer.py:132-136 of the reference: softmax(q^T k / 8) v, one
// image = one softmax domain), forward with the softmax statistics and backward.  Head-major rows (column c = h*64 + d); q, k, v, o, dO,
// dq, dk, dv are [N][*] with a row stride of their own (q | k | v may be three column blocks of one [N][768] buffer).  q is UNSCALED here:
// the kernels multiply by 1/8 on load (a power of two, exact), so the scores have the bits sig_attn_kernel (lt_attn.h) computes on
// pre-scaled q.  Tile sizes are the forward's: ATT_QT rows per block, ATT_KT staged rows, ATT_KS LDS row stride (lt_attn_parts.h).
//   ab_fwd_kernel     sig_attn_kernel's body (sig_attn_tile, lt_attn_parts.h) + lse [N][4] = m + logf(l) per (row, head)
//   ab_delta_kernel   delta [N][4] = sum_d dO[r][h][d] o[r][h][d]  (by the MFMA chain that contracts dP)
//   ab_dq_kernel      per (image, head, 128 queries), walking the image's keys:   dQ = (dS K) / 8
//   ab_dkv_kernel     per (image, head, 128 keys), walking the image's queries:   dV = P^T dO,  dK = dS^T (q / 8)
// with P = exp(S - lse) recomputed from q, k and lse, dP = dO V^T, dS = P * (dP - delta).  Nothing n x n reaches memory.
// Every contraction is exact-fp32 MFMA (v_mfma_f32_32x32x2_f32), natural-log scores and expf.  As in sig_attn_kernel a lane owns ONE
// column of a 32 x 32 score block and 16 of its rows, so the exponentiated block is, register for register, the B operand of the
// contraction that follows it and P / dS never leave the VGPRs.
// Summation order: a block walks the other side's rows in ascending tiles of 64, two chunks of 32 each; every chunk is an MFMA chain of
// its own started at zero (32 terms, in row order), and the chunks are added to the running sum in ascending order.  No floating-point
// atomics; every output row is written exactly once, by the one block that owns it: two calls give the same bits.  Rows beyond an image
// are staged as zeros and their P is set to zero explicitly (their lse is not defined); nothing beyond an image is loaded or stored.
// A block finds its (image, tile) by walking cu_sub: the grid is floor(N / 128) + n_images blocks per head, an upper bound of the
// tiles of any split of N rows into n_images images, so no image size has to be known on the host.
// The walk is serial in n_images and every block makes it, so the entry points bound n_images (4096): at that bound a block reads 16 KB
// of cu_sub through the scalar cache before it starts.
#pragma once
#include "lt_attn_parts.h"

namespace lt {

// block b of a head -> its image (first row n0, Ni rows) and the first row t0 of its tile within the image; false: no such tile
__device__ __forceinline__ bool ab_find_tile(const int* __restrict__ cu_sub, int n_images, int b, int& n0, int& Ni, int& t0) {
  int first = 0;
  for (int i = 0; i < n_images; ++i) {
    const int a = cu_sub[i], n = cu_sub[i + 1] - a;
    const int nt = n > 0 ? (n + ATT_QT - 1) / ATT_QT : 0;
    if (b < first + nt) {
      n0 = a; Ni = n; t0 = (b - first) * ATT_QT;
      return true;
    }
    first += nt;
  }
  return false;
}

// row of element r of a 32 x 32 MFMA result held by this lane (its column is lane & 31)
__device__ __forceinline__ int ab_row(int r, int h2) { return (r & 3) + 8 * (r >> 2) + 4 * h2; }

__device__ __forceinline__ void ab_zero(f32x16& a) {
#pragma unroll
  for (int r = 0; r < 16; ++r) a[r] = 0.f;
}

// acc[row][col] = sum_d T[row0 + row][d] * f[col][d]: T a staged tile (row stride ATT_KS), f the lane's own 64-channel fragment.
// PARTS = 1: one MFMA chain over the 64 channels, the forward's scores bit for bit.  PARTS = 4 (dP and delta): four chains of 16
// channels, each started at zero, added in channel order -- the difference dP - delta cancels most of either term, and a chain's
// rounding grows with its length (measured on the peaky family's two-row image: 1.2 x the bar with one chain, inside it with four).
template <int PARTS>
__device__ __forceinline__ void ab_rows_dot(const float* __restrict__ T, int row0, int lq, int h2, const f32x4 (&f)[8], f32x16& acc) {
  const float* tp = &T[(row0 + lq) * ATT_KS + h2 * 4];
#pragma unroll
  for (int p = 0; p < PARTS; ++p) {
    f32x16 part;
    ab_zero(part);
#pragma unroll
    for (int kk = p * (8 / PARTS); kk < (p + 1) * (8 / PARTS); ++kk) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(tp + kk * 8);
#pragma unroll
      for (int s = 0; s < 4; ++s) part = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], f[kk][s], part, 0, 0, 0);
    }
    if (p == 0) acc = part;
    else acc += part;
  }
}

// (o0 | o1)[d][col] += sum_row T[row0 + row][d] * w[row][col]: w the lane's 16 rows of a 32 x 32 block (P or dS), d = 0..31 | 32..63.
// The 32 rows are one chain started at zero, added to the running sum afterwards.
__device__ __forceinline__ void ab_cols_acc(const float* __restrict__ T, int row0, int lq, int h2, const f32x16& w, f32x16& o0, f32x16& o1) {
  f32x16 p0, p1;
  ab_zero(p0);
  ab_zero(p1);
  const float* tp = &T[(row0 + h2 * 4) * ATT_KS + lq];
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const float a0 = tp[(kk * 8 + s) * ATT_KS];
      const float a1 = tp[(kk * 8 + s) * ATT_KS + 32];
      p0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, w[kk * 4 + s], p0, 0, 0, 0);
      p1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, w[kk * 4 + s], p1, 0, 0, 0);
    }
  }
  o0 += p0;
  o1 += p1;
}

// rows r0 .. r0 + ATT_KT - 1 of one head of an image (base: its row 0, column 0 of the head) into a tile, times `scale`; rows at or
// beyond Ni are zeros and are not loaded
__device__ __forceinline__ void ab_stage(float* __restrict__ T, const float* __restrict__ base, int64_t ld, int r0, int Ni, float scale) {
  const int srow = threadIdx.x >> 4, sc4 = (threadIdx.x & 15) * 4;
#pragma unroll
  for (int i = 0; i < ATT_KT / 16; ++i) {
    const int r = srow + i * 16;
    f32x4 x = {0.f, 0.f, 0.f, 0.f};
    if (r0 + r < Ni) {
      x = *reinterpret_cast<const f32x4*>(base + (int64_t)(r0 + r) * ld + sc4);
#pragma unroll
      for (int e = 0; e < 4; ++e) x[e] *= scale;
    }
    *reinterpret_cast<f32x4*>(&T[r * ATT_KS + sc4]) = x;
  }
}

// the lane's 64-channel fragment of one row (p: the row's head, + 4 h2), times `scale`
__device__ __forceinline__ void ab_frag(const float* __restrict__ p, float scale, f32x4 (&f)[8]) {
#pragma unroll
  for (int kk = 0; kk < 8; ++kk) {
    f[kk] = *reinterpret_cast<const f32x4*>(p + kk * 8);
#pragma unroll
    for (int e = 0; e < 4; ++e) f[kk][e] *= scale;
  }
}

// ---------------------------------------------------------------------------------------------
// Forward with statistics: grid (floor(N / 128) + n_images, head), block 256.  sig_attn_tile<true> (lt_attn_parts.h), the body
// sig_attn_kernel runs as well: the message has the inference kernel's bits because both execute the same statements.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ab_fwd_kernel(const float* __restrict__ Q, int64_t ldq, const float* __restrict__ K, int64_t ldk,
                                                     const float* __restrict__ V, int64_t ldv, const int* __restrict__ cu_sub, int n_images,
                                                     float* __restrict__ out, int64_t ldo, float* __restrict__ lse /*[N][4]*/) {
  int n0, Ni, q0;
  if (!ab_find_tile(cu_sub, n_images, blockIdx.x, n0, Ni, q0)) return;
  sig_attn_tile<true>(Q, ldq, K, ldk, V, ldv, n0, Ni, q0, blockIdx.y, out, ldo, lse);
}

// ---------------------------------------------------------------------------------------------
// delta [N][4]: grid (cdiv(N, 32), head), block 64.  The diagonal of the 32 x 32 block O dO^T, contracted by the very MFMA chain that
// contracts dP = dO V^T in the two kernels below (same channel order, the two factors of a product swapped at most), so that where
// o = v bit for bit (an image of one sub-line) dP - delta is exactly zero.  Rows are rows of the batch: no image enters.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void ab_delta_kernel(const float* __restrict__ dO, int64_t ldg, const float* __restrict__ O, int64_t ldo,
                                                      int64_t N, float* __restrict__ delta) {
  __shared__ __attribute__((aligned(16))) float Os[32 * ATT_KS];
  const int head = blockIdx.y, lane = threadIdx.x, h2 = lane >> 5, lq = lane & 31;
  const int64_t r0 = (int64_t)blockIdx.x * 32;
  const int srow = lane >> 4, sc4 = (lane & 15) * 4;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int r = srow + i * 4;
    f32x4 x = {0.f, 0.f, 0.f, 0.f};
    if (r0 + r < N) x = *reinterpret_cast<const f32x4*>(O + (r0 + r) * ldo + head * DH + sc4);
    *reinterpret_cast<f32x4*>(&Os[r * ATT_KS + sc4]) = x;
  }
  const int64_t row = r0 + lq < N ? r0 + lq : N - 1;
  f32x4 gf[8];
  ab_frag(dO + row * ldg + head * DH + h2 * 4, 1.f, gf);
  __syncthreads();
  f32x16 acc;
  ab_rows_dot<4>(Os, 0, lq, h2, gf, acc);
  // element (row lq, column lq) sits in the half h2 = bit 2 of lq, register (lq & 3) + 4 (lq >> 3)
  float dg = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r)
    if (r == (lq & 3) + 4 * (lq >> 3)) dg = acc[r];
  if (h2 == ((lq >> 2) & 1) && r0 + lq < N) delta[(r0 + lq) * HEADS + head] = dg;
}

// ---------------------------------------------------------------------------------------------
// dQ: grid (floor(N / 128) + n_images, head), block 256; wave w owns 32 queries, a lane one of them (its q / 8 and dO rows, lse and
// delta in VGPRs).  Per 32-key chunk:  S^T = K (q/8)^T,  P^T = exp(S^T - lse),  dP^T = V dO^T,  dS^T = P^T (dP^T - delta),
// dQ^T += K^T dS^T.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ab_dq_kernel(const float* __restrict__ Q, int64_t ldq, const float* __restrict__ K, int64_t ldk,
                                                    const float* __restrict__ V, int64_t ldv, const float* __restrict__ dO, int64_t ldg,
                                                    const float* __restrict__ lse, const float* __restrict__ delta,
                                                    const int* __restrict__ cu_sub, int n_images, float* __restrict__ dQ, int64_t lddq) {
  __shared__ __attribute__((aligned(16))) float Ks[ATT_KT * ATT_KS];
  __shared__ __attribute__((aligned(16))) float Vs[ATT_KT * ATT_KS];
  const int head = blockIdx.y;
  int n0, Ni, q0;
  if (!ab_find_tile(cu_sub, n_images, blockIdx.x, n0, Ni, q0)) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int h2 = lane >> 5, lq = lane & 31;
  const int q = q0 + wave * 32 + lq;
  const bool wave_active = q0 + wave * 32 < Ni;  // wave-uniform
  const int64_t qrow = n0 + (q < Ni ? q : Ni - 1);   // a lane behind the image repeats its last query; it stores nothing

  f32x4 qf[8], gf[8];
  ab_frag(Q + qrow * ldq + head * DH + h2 * 4, 0.125f, qf);
  ab_frag(dO + qrow * ldg + head * DH + h2 * 4, 1.f, gf);
  const float lse_q = lse[qrow * HEADS + head], delta_q = delta[qrow * HEADS + head];
  f32x16 o0, o1;
  ab_zero(o0);
  ab_zero(o1);

  const float* kbase = K + (int64_t)n0 * ldk + head * DH;
  const float* vbase = V + (int64_t)n0 * ldv + head * DH;
  for (int t0 = 0; t0 < Ni; t0 += ATT_KT) {
    __syncthreads();
    ab_stage(Ks, kbase, ldk, t0, Ni, 1.f);
    ab_stage(Vs, vbase, ldv, t0, Ni, 1.f);
    __syncthreads();
    if (!wave_active) continue;
#pragma unroll
    for (int c = 0; c < ATT_KT / 32; ++c) {
      const int kv0 = t0 + c * 32;
      if (kv0 >= Ni) break;
      f32x16 st, dp;
      ab_rows_dot<1>(Ks, c * 32, lq, h2, qf, st);
      ab_rows_dot<4>(Vs, c * 32, lq, h2, gf, dp);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float p = kv0 + ab_row(r, h2) < Ni ? expf(st[r] - lse_q) : 0.f;   // keys beyond the image: P = 0, as in the forward
        st[r] = p * (dp[r] - delta_q);
      }
      ab_cols_acc(Ks, c * 32, lq, h2, st, o0, o1);
    }
  }
  if (wave_active && q < Ni) {
    float* op = dQ + (int64_t)(n0 + q) * lddq + head * DH;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int d = ab_row(r, h2);
      op[d] = o0[r] * 0.125f;
      op[d + 32] = o1[r] * 0.125f;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// dK and dV (either may be NULL): grid (floor(N / 128) + n_images, head), block 256; wave w owns 32 keys, a lane one of them (its k and
// v rows in VGPRs).  Per 32-query chunk of the staged q / 8, dO, lse and delta:  S = (q/8) K^T,  P = exp(S - lse) (0 for a query or a
// key beyond the image),  dV^T += dO^T P,  dP = dO V^T,  dS = P (dP - delta),  dK^T += (q/8)^T dS.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ab_dkv_kernel(const float* __restrict__ Q, int64_t ldq, const float* __restrict__ K, int64_t ldk,
                                                     const float* __restrict__ V, int64_t ldv, const float* __restrict__ dO, int64_t ldg,
                                                     const float* __restrict__ lse, const float* __restrict__ delta,
                                                     const int* __restrict__ cu_sub, int n_images, float* __restrict__ dK, int64_t lddk,
                                                     float* __restrict__ dV, int64_t lddv) {
  __shared__ __attribute__((aligned(16))) float Qs[ATT_KT * ATT_KS];
  __shared__ __attribute__((aligned(16))) float Gs[ATT_KT * ATT_KS];
  __shared__ float Ls[ATT_KT], Ds[ATT_KT];
  const int head = blockIdx.y;
  int n0, Ni, k0;
  if (!ab_find_tile(cu_sub, n_images, blockIdx.x, n0, Ni, k0)) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h2 = lane >> 5, lq = lane & 31;
  const int kv = k0 + wave * 32 + lq;
  const bool wave_active = k0 + wave * 32 < Ni;  // wave-uniform
  const bool kv_in = kv < Ni;
  const int64_t krow = n0 + (kv_in ? kv : Ni - 1);
  const bool want_dk = dK != nullptr;

  f32x4 kf[8], vf[8];
  ab_frag(K + krow * ldk + head * DH + h2 * 4, 1.f, kf);
  if (want_dk) ab_frag(V + krow * ldv + head * DH + h2 * 4, 1.f, vf);
  f32x16 dk0, dk1, dv0, dv1;
  ab_zero(dk0);
  ab_zero(dk1);
  ab_zero(dv0);
  ab_zero(dv1);

  const float* qbase = Q + (int64_t)n0 * ldq + head * DH;
  const float* gbase = dO + (int64_t)n0 * ldg + head * DH;
  for (int t0 = 0; t0 < Ni; t0 += ATT_KT) {
    __syncthreads();
    ab_stage(Qs, qbase, ldq, t0, Ni, 0.125f);
    ab_stage(Gs, gbase, ldg, t0, Ni, 1.f);
    if (tid < ATT_KT) {
      const bool in = t0 + tid < Ni;
      Ls[tid] = in ? lse[(int64_t)(n0 + t0 + tid) * HEADS + head] : 0.f;
      Ds[tid] = in ? delta[(int64_t)(n0 + t0 + tid) * HEADS + head] : 0.f;
    }
    __syncthreads();
    if (!wave_active) continue;
#pragma unroll
    for (int c = 0; c < ATT_KT / 32; ++c) {
      const int q0 = t0 + c * 32;
      if (q0 >= Ni) break;
      f32x16 st;
      ab_rows_dot<1>(Qs, c * 32, lq, h2, kf, st);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int qr = ab_row(r, h2);
        // a query beyond the image has no lse: its P is zero by decree, not by 0 * exp(garbage)
        st[r] = (q0 + qr < Ni && kv_in) ? expf(st[r] - Ls[c * 32 + qr]) : 0.f;
      }
      if (dV) ab_cols_acc(Gs, c * 32, lq, h2, st, dv0, dv1);
      if (want_dk) {
        f32x16 dp;
        ab_rows_dot<4>(Gs, c * 32, lq, h2, vf, dp);
#pragma unroll
        for (int r = 0; r < 16; ++r) st[r] = st[r] * (dp[r] - Ds[c * 32 + ab_row(r, h2)]);
        ab_cols_acc(Qs, c * 32, lq, h2, st, dk0, dk1);
      }
    }
  }
  if (wave_active && kv_in) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int d = ab_row(r, h2);
      if (want_dk) {
        float* op = dK + (int64_t)(n0 + kv) * lddk + head * DH;
        op[d] = dk0[r];
        op[d + 32] = dk1[r];
      }
      if (dV) {
        float* op = dV + (int64_t)(n0 + kv) * lddv + head * DH;
        op[d] = dv0[r];
        op[d + 32] = dv1[r];
      }
    }
  }
}

}  // namespace lt
