// The backward of a point-wise linear layer (Conv1d(k=1) / Linear: Y = X W^T + b, every weight of the network, stated on the UNFOLDED
// state_dict weights) and the descriptor head on top of it (models/line_transformer.py:245-246 of the reference:
// line_desc = F.normalize(final_proj(x), p=2, dim=1)), forward and backward.  rows = B n positions, row-major [rows][C] activations
// (the layout linetr_forward* writes).
//   lb_fwd_kernel<HEAD>   Y = act(X W^T + b).  HEAD (N = K = 256): a block owns 32 whole rows, so the epilogue normalises them,
//                         d = y / max(|y|, 1e-12), and, given an upstream g, also takes the normalisation's backward
//                         gy = (g - d (d . g)) / max(|y|, 1e-12)   (|y| < 1e-12: gy = g / 1e-12, what clamp_min's backward leaves);
//                         y itself never reaches memory.
//   lb_dx_kernel          dX [rows][K] = G' [rows][N] W [N][K];  G' = G with the entries zeroed where the mask (the layer's own
//                         post-ReLU output, handed in by the caller) is <= 0.  Nothing is recomputed to decide a sign.
//   lb_dw_partial_kernel  one block per (chunk of LB_CHUNK rows, 64 of N, 64 of K): its tile of G'^T X, and (the blocks of the first
//                         K tile) its 64 column sums of G', to the workspace;
//   lb_dw_reduce_kernel   dW [N][K] and db [N]: the chunks added in ascending chunk order.
// Every contraction is exact-fp32 MFMA (v_mfma_f32_32x32x2_f32, as the matcher's dot_tile_64x64): a gradient does not inherit a split's
// error.  Deterministic: no floating-point atomics, the chunk size is a compile-time constant and every sum has a fixed order, so two
// calls give the same bits; every output element is written.  Rows beyond `rows` are never loaded or stored (a tile's tail is zeros).
#pragma once
#include "lt_common.h"

namespace lt {

constexpr int LB_CHUNK = 256;          // rows of one chunk of the weight gradient's row reduction
constexpr int LB_KS = 32;              // contraction step of a tile
constexpr int LB_LS_CC = 36;           // LDS row stride of an operand tile held [out index][contraction]
constexpr float LB_EPS = 1e-12f;       // F.normalize's eps
constexpr int LB_HEAD_ROWS = 32;       // rows of a head block

// An operand of a tile product, seen as E(o, c): o its output index (a row or a column of the result), c the contraction index.
//   CM = false: E(o, c) = P[o ld + c]  (the contraction runs along the memory rows:    X and W of the forward, G of dX)
//   CM = true:  E(o, c) = P[c ld + o]  (the contraction runs across the memory rows:   W of dX, G and X of dW)
// The tile covers o0 .. o0 + T - 1 and LB_KS contraction indices from c0; whatever lies at or beyond o_lim / c_lim is zero and is not
// loaded (the limits along a memory row are multiples of 4: a 16-byte piece is inside or outside as a whole).  M: the mask of P, or NULL.
template <bool CM, int T>
struct LbOperand {
  static constexpr int PIECES = T / 32;                    // 16-byte pieces per thread of 256
  static constexpr int LS = CM ? T + 8 : LB_LS_CC;         // CM: rows 4 apart (the two k of an MFMA) fall into different bank halves
  static constexpr int FLOATS = CM ? LB_KS * LS : T * LS;
  f32x4 v[PIECES];

  __device__ __forceinline__ void fetch(const float* __restrict__ P, const float* __restrict__ M, int64_t ld, int64_t o0, int64_t o_lim,
                                        int64_t c0, int64_t c_lim) {
#pragma unroll
    for (int i = 0; i < PIECES; ++i) {
      const int p = threadIdx.x + i * 256;
      int64_t o, c, at;
      if constexpr (CM) { c = c0 + p / (T / 4); o = o0 + (p % (T / 4)) * 4; at = c * ld + o; }
      else { o = o0 + (p >> 3); c = c0 + (p & 7) * 4; at = o * ld + c; }
      f32x4 x = f32x4{0.f, 0.f, 0.f, 0.f};
      if (o < o_lim && c < c_lim) {
        x = *reinterpret_cast<const f32x4*>(P + at);
        if (M) {
          const f32x4 m = *reinterpret_cast<const f32x4*>(M + at);
#pragma unroll
          for (int e = 0; e < 4; ++e) x[e] = m[e] > 0.f ? x[e] : 0.f;
        }
      }
      v[i] = x;
    }
  }
  __device__ __forceinline__ void stage(float* __restrict__ S) const {
#pragma unroll
    for (int i = 0; i < PIECES; ++i) {
      const int p = threadIdx.x + i * 256;
      if constexpr (CM) *reinterpret_cast<f32x4*>(&S[(p / (T / 4)) * LS + (p % (T / 4)) * 4]) = v[i];
      else *reinterpret_cast<f32x4*>(&S[(p >> 3) * LS + (p & 7) * 4]) = v[i];
    }
  }
  // the four values E(o, kk 8 + half 4 + s), s = 0 .. 3, of this lane's output index o (within the tile)
  static __device__ __forceinline__ f32x4 read(const float* __restrict__ S, int o, int kk, int half) {
    if constexpr (CM) {
      const float* q = &S[(kk * 8 + half * 4) * LS + o];
      return f32x4{q[0], q[LS], q[2 * LS], q[3 * LS]};
    } else {
      return *reinterpret_cast<const f32x4*>(&S[o * LS + kk * 8 + half * 4]);
    }
  }
};

// element r of a 32 x 32 MFMA result: row lb_acc_row(r, lane), column lane & 31
__device__ __forceinline__ int lb_acc_row(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

__device__ __forceinline__ void lb_zero(f32x16& a) {
#pragma unroll
  for (int r = 0; r < 16; ++r) a[r] = 0.f;
}

// acc[nb] += the 32 x 32 block (rows wm 32 .., columns (wn NB + nb) 32 ..) of  sum_c A(a, c) B(b, c)  over c_begin <= c < c_end, for a
// block of 256 threads = WM x WN waves: an (WM 32) x (WN NB 32) tile.  The next contraction step travels in registers while the
// current one is multiplied.  Every step of LB_KS indices is a chain of its own, started at zero, and the steps are added in order: a
// contraction over 1024 indices then rounds like 32 sums of 32 terms, not like one chain of 1024 (whose error grows with its length
// and was measured above four times that of a float32 torch product at K = 1024).
template <bool ACM, bool BCM, int WM, int WN, int NB>
__device__ __forceinline__ void lb_tile(f32x16 (&acc)[NB], const float* __restrict__ A, const float* __restrict__ Amask, int64_t lda,
                                        int64_t a0, int64_t a_lim, const float* __restrict__ B, int64_t ldb, int64_t b0, int64_t b_lim,
                                        int64_t c_begin, int64_t c_end, float* __restrict__ As, float* __restrict__ Bs) {
  static_assert(WM * WN == 4, "four waves");
  using OpA = LbOperand<ACM, WM * 32>;
  using OpB = LbOperand<BCM, WN * NB * 32>;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = wave / WN, wn = wave % WN, half = lane >> 5, l32 = lane & 31;
  OpA ra;
  OpB rb;
  ra.fetch(A, Amask, lda, a0, a_lim, c_begin, c_end);
  rb.fetch(B, nullptr, ldb, b0, b_lim, c_begin, c_end);
  for (int64_t c0 = c_begin; c0 < c_end; c0 += LB_KS) {
    __syncthreads();                                       // the step before has been read
    ra.stage(As);
    rb.stage(Bs);
    if (c0 + LB_KS < c_end) {
      ra.fetch(A, Amask, lda, a0, a_lim, c0 + LB_KS, c_end);
      rb.fetch(B, nullptr, ldb, b0, b_lim, c0 + LB_KS, c_end);
    }
    __syncthreads();
    f32x16 part[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) lb_zero(part[nb]);
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const f32x4 a = OpA::read(As, wm * 32 + l32, kk, half);
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        const f32x4 b = OpB::read(Bs, (wn * NB + nb) * 32 + l32, kk, half);
#pragma unroll
        for (int s = 0; s < 4; ++s) part[nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], b[s], part[nb], 0, 0, 0);
      }
    }
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) acc[nb] += part[nb];
  }
}

// HEAD = false: grid (cdiv(rows, 64), N / 64), a 64 x 64 tile of Y [rows][ldy] = act(X W^T + b); act 1: ReLU; b may be NULL.
// HEAD = true:  grid (cdiv(rows, 32)), N = K = 256, every stride 256: rows r0 .. r0 + 31 of desc = y / max(|y|, eps) (Y, may be NULL)
//               and, given g, of gy (may be NULL without g).
template <bool HEAD>
__global__ __launch_bounds__(256) void lb_fwd_kernel(const float* __restrict__ X, int64_t ldx, const float* __restrict__ W,
                                                     const float* __restrict__ bias, int64_t rows, int N, int K, int act,
                                                     float* __restrict__ Y, int64_t ldy, const float* __restrict__ g,
                                                     float* __restrict__ gy) {
  constexpr int WM = HEAD ? 1 : 2, WN = HEAD ? 4 : 2, NB = HEAD ? 2 : 1;
  __shared__ __attribute__((aligned(16))) float As[LbOperand<false, WM * 32>::FLOATS];
  __shared__ __attribute__((aligned(16))) float Bs[LbOperand<false, WN * NB * 32>::FLOATS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wm = wave / WN, wn = wave % WN;
  const int64_t r0 = (int64_t)blockIdx.x * (WM * 32);
  const int n0 = HEAD ? 0 : blockIdx.y * 64;
  f32x16 acc[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) lb_zero(acc[nb]);
  lb_tile<false, false, WM, WN, NB>(acc, X, nullptr, ldx, r0, rows, W, K, n0, N, 0, K, As, Bs);
  int col[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    col[nb] = n0 + (wn * NB + nb) * 32 + (lane & 31);
    const float b = bias ? bias[col[nb]] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float y = acc[nb][r] + b;
      acc[nb][r] = act ? fmaxf(y, 0.f) : y;
    }
  }
  if constexpr (!HEAD) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t row = r0 + wm * 32 + lb_acc_row(r, lane);
      if (row < rows) Y[row * ldy + col[0]] = acc[0][r];
    }
  } else {
    // |y|^2 and y . g of a row: the lane's two columns, the 32 lanes of its half (xor butterfly), then the four waves in wave order
    __shared__ float s_yy[4][LB_HEAD_ROWS], s_yg[4][LB_HEAD_ROWS];
    float gv[NB][16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int lr = lb_acc_row(r, lane);
      const int64_t row = r0 + lr;
      float yy = 0.f, yg = 0.f;
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        gv[nb][r] = (g && row < rows) ? g[row * D + col[nb]] : 0.f;
        yy = fmaf(acc[nb][r], acc[nb][r], yy);
        yg = fmaf(acc[nb][r], gv[nb][r], yg);
      }
#pragma unroll
      for (int o = 16; o > 0; o >>= 1) {
        yy += __shfl_xor(yy, o, 64);
        yg += __shfl_xor(yg, o, 64);
      }
      if ((lane & 31) == 0) { s_yy[wave][lr] = yy; s_yg[wave][lr] = yg; }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int lr = lb_acc_row(r, lane);
      const int64_t row = r0 + lr;
      if (row >= rows) continue;
      const float yy = ((s_yy[0][lr] + s_yy[1][lr]) + s_yy[2][lr]) + s_yy[3][lr];
      const float yg = ((s_yg[0][lr] + s_yg[1][lr]) + s_yg[2][lr]) + s_yg[3][lr];
      const float norm = sqrtf(yy), c = fmaxf(norm, LB_EPS);
      const bool through = norm >= LB_EPS;                 // clamp_min's backward passes the norm's gradient only here
      const float dg = yg / c;
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        const float d = acc[nb][r] / c;
        if (Y) Y[row * D + col[nb]] = d;
        if (gy) gy[row * D + col[nb]] = through ? (gv[nb][r] - d * dg) / c : gv[nb][r] / c;
      }
    }
  }
}

// grid (cdiv(rows, 64), cdiv(K, 64)): a 64 x 64 tile of dX [rows][ldx] = G' W.  G, mask: [rows][ldg]; W: [N][K].
__global__ __launch_bounds__(256) void lb_dx_kernel(const float* __restrict__ G, const float* __restrict__ mask, int64_t ldg,
                                                    const float* __restrict__ W, int64_t rows, int N, int K, float* __restrict__ dX,
                                                    int64_t ldx) {
  __shared__ __attribute__((aligned(16))) float As[LbOperand<false, 64>::FLOATS];
  __shared__ __attribute__((aligned(16))) float Bs[LbOperand<true, 64>::FLOATS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wm = wave >> 1, wn = wave & 1;
  const int64_t r0 = (int64_t)blockIdx.x * 64;
  const int k0 = blockIdx.y * 64;
  f32x16 acc[1];
  lb_zero(acc[0]);
  lb_tile<false, true, 2, 2, 1>(acc, G, mask, ldg, r0, rows, W, K, k0, K, 0, N, As, Bs);
  const int col = k0 + wn * 32 + (lane & 31);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t row = r0 + wm * 32 + lb_acc_row(r, lane);
    if (row < rows && col < K) dX[row * ldx + col] = acc[0][r];
  }
}

// grid (chunks, N / 64, cdiv(K, 64)), chunks = cdiv(rows, LB_CHUNK).  dw_part [chunks][N][K]: the block's tile of G'^T X over the rows
// of its chunk; db_part [chunks][N]: the column sums of G' over them, in row order, by the blocks of the first K tile.  Either may
// be NULL.
__global__ __launch_bounds__(256) void lb_dw_partial_kernel(const float* __restrict__ G, const float* __restrict__ mask, int64_t ldg,
                                                            const float* __restrict__ X, int64_t ldx, int64_t rows, int N, int K,
                                                            float* __restrict__ dw_part, float* __restrict__ db_part) {
  __shared__ __attribute__((aligned(16))) float As[LbOperand<true, 64>::FLOATS];
  __shared__ __attribute__((aligned(16))) float Bs[LbOperand<true, 64>::FLOATS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wm = wave >> 1, wn = wave & 1;
  const int64_t chunk = blockIdx.x, c_begin = chunk * LB_CHUNK, c_end = c_begin + LB_CHUNK < rows ? c_begin + LB_CHUNK : rows;
  const int n0 = blockIdx.y * 64, k0 = blockIdx.z * 64;
  if (dw_part) {
    f32x16 acc[1];
    lb_zero(acc[0]);
    lb_tile<true, true, 2, 2, 1>(acc, G, mask, ldg, n0, N, X, ldx, k0, K, c_begin, c_end, As, Bs);
    const int col = k0 + wn * 32 + (lane & 31);
    float* out = dw_part + chunk * N * K;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = n0 + wm * 32 + lb_acc_row(r, lane);
      if (col < K) out[(int64_t)row * K + col] = acc[0][r];
    }
  }
  if (db_part && blockIdx.z == 0) {
    // four row phases per column (one per wave, rows wave, wave + 4, ..), added in phase order
    __shared__ float s_db[4][64];
    const int n = n0 + lane;
    float s = 0.f;
    for (int64_t r = c_begin + wave; r < c_end; r += 4) {
      const float gv = G[r * ldg + n];
      s += (!mask || mask[r * ldg + n] > 0.f) ? gv : 0.f;
    }
    __syncthreads();
    s_db[wave][lane] = s;
    __syncthreads();
    if (wave == 0) db_part[chunk * N + n] = ((s_db[0][lane] + s_db[1][lane]) + s_db[2][lane]) + s_db[3][lane];
  }
}

// one thread per four elements of dW (N K / 4 of them), then of db (N / 4): the chunks in ascending order.  dW / db may be NULL.
__global__ __launch_bounds__(256) void lb_dw_reduce_kernel(const float* __restrict__ dw_part, const float* __restrict__ db_part, int chunks,
                                                           int N, int K, float* __restrict__ dW, float* __restrict__ db) {
  const int64_t nw = dW ? (int64_t)N * K / 4 : 0, nb = db ? N / 4 : 0;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nw + nb) return;
  const bool w = i < nw;
  const float* src = w ? dw_part + i * 4 : db_part + (i - nw) * 4;
  const int64_t step = w ? (int64_t)N * K : N;
  f32x4 s = *reinterpret_cast<const f32x4*>(src);
  for (int c = 1; c < chunks; ++c) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(src + c * step);
#pragma unroll
    for (int e = 0; e < 4; ++e) s[e] += v[e];
  }
  *reinterpret_cast<f32x4*>(w ? dW + i * 4 : db + (i - nw) * 4) = s;
}

}  // namespace lt
