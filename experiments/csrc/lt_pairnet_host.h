// Experiments build: the host entry points of the single-pair persistent signature network (lt_pairnet.h), defined in
// linetr_pair.hip and called by the forward pass's experiments hooks (lt_x_net.h).  No kernels here.
//   pairnet_fits      does this batch take the path (precision, image count, row count)?  h_cu may be NULL (size check only)
//   pairnet_ws_bytes  bytes of workspace it needs for N rows (0 when N is out of range)
//   pairnet_prepare   zeroes the arrival counters on the stream (call it EARLY, well ahead of the launch)
//   pairnet_run       z0 [N,256] -> line_desc [N,256]
#pragma once
#include "lt_handle.h"

namespace lt {

constexpr int PN_MAX_ROWS = 1024;
bool pairnet_fits(LinetrHandle* h, int n_images, int N, const int32_t* h_cu);
int64_t pairnet_ws_bytes(const LinetrHandle* h, int N);
int pairnet_prepare(LinetrHandle* h, hipStream_t st, int N, void* ws);
int pairnet_run(LinetrHandle* h, hipStream_t st, const float* z0, float* out, const int32_t* h_cu, int n_images, int N, void* ws);

}  // namespace lt
