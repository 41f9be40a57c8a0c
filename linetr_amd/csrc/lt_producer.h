// Fused SuperPoint head post-processing: turns the two raw head outputs into the dense maps
// the line tokeniser consumes, in the layout it wants.
//   score head  models/superpoint.py:161-167   softmax over 65 channels, drop the dustbin, depth-to-space (8x8 cells)
//   desc head   models/superpoint.py:190-193   F.normalize(p=2, dim=1) -- here fused with the NCHW -> NHWC transposition
//                                              that linetr_describe otherwise does in a separate pass
// Both kernels are HBM-bound by design: every input byte is read once, every output byte written once.
#pragma once
#include "lt_common.h"

namespace lt {

// One block = CELLS consecutive cells (h*Wc + w) of one image x all 256 channels.  LDS tile [256][CELLS + 1]: the odd
// stride makes the NCHW-side accesses (lanes along cells) and the NHWC-side accesses (lanes along channels) both
// bank-conflict-free.  CELLS = 32 (33 KiB of LDS, 4 blocks per CU) keeps more loads in flight than 64 (2 blocks per
// CU): 5.4 vs 4.3 TB/s on a cfg3-sized batch (tools/producer_bench.py).
// ROWS: the raw head output is channel-last rows [B * HW][ld >= 256] (linetr_superpoint_heads_rows: what the native encoder's convDb
// writes) instead of NCHW; only phase 1 differs, so given the same values both layouts give the same bits.
// The kernels' text is lt_producer_body.h, included once for float32 and once for the other element types.
#define LT_HEAD_DESC_TEMPLATE template <int CELLS, bool ROWS>
#define LT_HEAD_DESC_KERNEL sp_desc_head_kernel
#define LT_HEAD_SCORE_TEMPLATE template <bool ROWS>
#define LT_HEAD_SCORE_KERNEL sp_score_head_kernel
#define LT_HEAD_EI float
#define LT_HEAD_EO float
#define LT_HEAD_LD_PARAM , int64_t ld
#define LT_HEAD_DESC_PROLOGUE typedef float EI; typedef float EO;
#define LT_HEAD_SCORE_PROLOGUE typedef float EI;
#include "lt_producer_body.h"
#undef LT_HEAD_DESC_TEMPLATE
#undef LT_HEAD_DESC_KERNEL
#undef LT_HEAD_SCORE_TEMPLATE
#undef LT_HEAD_SCORE_KERNEL
#undef LT_HEAD_EI
#undef LT_HEAD_EO
#undef LT_HEAD_LD_PARAM
#undef LT_HEAD_DESC_PROLOGUE
#undef LT_HEAD_SCORE_PROLOGUE

// NCHW raw head outputs of type TI, descriptor maps of type TO (linetr_superpoint_heads_typed; not both float: those are the kernels above)
#define LT_HEAD_DESC_TEMPLATE template <int CELLS, class TI, class TO>
#define LT_HEAD_DESC_KERNEL sp_desc_head_typed_kernel
#define LT_HEAD_SCORE_TEMPLATE template <class TI>
#define LT_HEAD_SCORE_KERNEL sp_score_head_typed_kernel
#define LT_HEAD_EI TI
#define LT_HEAD_EO TO
#define LT_HEAD_LD_PARAM
#define LT_HEAD_SCORE_PROLOGUE typedef TI EI; constexpr bool ROWS = false; constexpr int64_t ld = 0; (void)ld;
#define LT_HEAD_DESC_PROLOGUE LT_HEAD_SCORE_PROLOGUE typedef TO EO;
#include "lt_producer_body.h"
#undef LT_HEAD_DESC_TEMPLATE
#undef LT_HEAD_DESC_KERNEL
#undef LT_HEAD_SCORE_TEMPLATE
#undef LT_HEAD_SCORE_KERNEL
#undef LT_HEAD_EI
#undef LT_HEAD_EO
#undef LT_HEAD_LD_PARAM
#undef LT_HEAD_DESC_PROLOGUE
#undef LT_HEAD_SCORE_PROLOGUE

}  // namespace lt
