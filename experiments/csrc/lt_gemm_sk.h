// Experiments build only: the launcher of the stream-K tail of the pipelined 128x256 tile.  The kernel is the SKT
// instantiation of gemm_split_kernel (lt_gemm_split.h), which only this file instantiates.
//
// When the last round of 128x256 tiles would leave a good part of the chip idle, those tiles are shared by one block per CU
// instead (see the kernel).  Measured quantisation: 25472 x 512 x 512 (398 tiles) took as long as 32768 x 512 x 512 (512 tiles),
// 104 us.
// OFF by default (LINETR_STREAMK=1 turns it on, read per launch so that the tests can exercise it): the stream-K kernel is
// correct and deterministic (test_experiments.py::test_gemm_stream_k_tail) but as built it LOSES -- 25472x512x512 110 us vs
// 92 us, 25472x768x256 114 us vs 82 us -- because the segment loop's extra state spills 60 VGPRs and 70 SGPRs next to the
// 256-register pipelined main loop, which slows the data-parallel tiles of the same launch as well.  Kept as the starting
// point for a leaner version.
#pragma once
#include "lt_gemm_split.h"

namespace lt {

// Does a tail pay for this 128x256-tile GEMM?  Only when >= 3/16 (5/16 for a single round) of the CUs would idle in the last
// round and the tail has enough K tiles to share.
inline bool gemm_split_sk_pays(const GemmArgs& g, int groups) {
  const int n_cu = cu_count();
  const int T = (g.N / 256) * cdiv(g.M, 128), nkw = g.K / 32;
  const int full = T / n_cu * n_cu, rem = T - full;
  const int idle_ok = full > 0 ? n_cu * 13 / 16 : n_cu * 11 / 16;
  return groups == 1 && SplitTileLds<128, 256, 3, true>::wide_epi(g) && rem > 0 && rem <= idle_ok && (int64_t)rem * nkw >= 2 * n_cu &&
         n_cu <= 256 && nkw <= 4096;
}

// ws: [CUs][128 * 256] floats; flags: [CUs + 1], zeroed once; epoch: a value no earlier launch on them has used
template <int PL, int FMT>
inline int gemm_split_sk_launch(const SplitGemmArgs& sa, float* ws, unsigned* flags, unsigned epoch, hipStream_t st) {
  constexpr int BM = 128, BN = 256, WM = 2, WN = 4;
  using Lds = SplitTileLds<BM, BN, PL, true>;
  const int n_cu = cu_count(), T = (sa.g.N / BN) * cdiv(sa.g.M, BM);
  SplitGemmArgs sa2 = sa;
  sa2.wide_epi = 1;
  sa2.sk_first = T / n_cu * n_cu; sa2.sk_blocks = n_cu; sa2.sk_ws = ws; sa2.sk_flags = flags; sa2.sk_epoch = epoch;
  // the stream-K kernel is its own instantiation with one register set of prefetch (PFD = 1): with two, the segment
  // loop's extra state spilled 116 VGPRs
  LT_HIP((allow_dynamic_lds<gemm_split_kernel<BM, BN, WM, WN, PL, true, FMT, 1, true, true>>((int)Lds::bytes)));
  hipLaunchKernelGGL((gemm_split_kernel<BM, BN, WM, WN, PL, true, FMT, 1, true, true>), dim3(sa2.sk_first + n_cu), dim3(WM * WN * 64),
                     Lds::bytes, st, sa2);
  LT_LAUNCH_CHECK();
  return 0;
}

}  // namespace lt
