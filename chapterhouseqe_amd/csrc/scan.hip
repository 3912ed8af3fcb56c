// scan.hip -- the tiled exclusive scan of a uint32_t array into 32-bit offsets (gfx950, wave64), shared by the join (matches
// per left row, FULL's unmatched right rows: join.cpp) and the string functions (row lengths: filter.cpp).  Three launches
// that hand data over only at launch boundaries: the 64-bit sum of every tile, the scan of the sums by one workgroup (the
// 64-bit total behind them), the offsets of every tile.  Parameters: typed_ops.h.
#include <hip/hip_runtime.h>

#include "join_device.h"
#include "scan_device.h"
#include "strfn_device.h"
#include "typed_ops.h"

namespace chq {
namespace {

static_assert(kJoinTile == kScanTile && STRFN_SCAN_CHUNK == kScanTile, "the callers count ntiles in tiles of their own name");

__global__ __launch_bounds__(kScanBlock) void scan_tile_sums_kernel(const OffsetsScanParams p) {
  __shared__ uint64_t sums[kScanWaves];
  const int64_t i0 = (int64_t)blockIdx.x * kScanTile + threadIdx.x;
  uint64_t v = 0;
#pragma unroll
  for (int k = 0; k < kScanItems; ++k)
    if (i0 + k * kScanBlock < p.n) v += p.len[i0 + k * kScanBlock];
  const uint64_t tot = block_sum<uint64_t>(v, sums);
  if (threadIdx.x == 0) p.tile_sums[blockIdx.x] = tot;
}

// one workgroup, in 64 bits: 65 536 x 65 536 equal join keys are 2^32 output rows, and the total must not wrap
__global__ __launch_bounds__(kScanBlock) void scan_totals_kernel(const OffsetsScanParams p) {
  __shared__ uint64_t sums[kScanWaves];
  scan_totals_in_place<uint64_t>(p.tile_sums, p.ntiles, p.tile_sums + p.ntiles, sums);
}

// out[i] = tile prefix + prefix inside the tile, mod 2^32; a thread takes kScanItems consecutive items
__global__ __launch_bounds__(kScanBlock) void scan_offsets_kernel(const OffsetsScanParams p) {
  __shared__ uint32_t sums[kScanWaves];
  const int64_t i0 = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanItems;
  uint32_t c[kScanItems], v = 0;
#pragma unroll
  for (int k = 0; k < kScanItems; ++k) {
    c[k] = i0 + k < p.n ? p.len[i0 + k] : 0u;
    v += c[k];
  }
  uint32_t tot;
  uint32_t at = block_exclusive_scan<uint32_t>(v, sums, &tot) + (uint32_t)p.tile_sums[blockIdx.x];
#pragma unroll
  for (int k = 0; k < kScanItems; ++k) {
    if (i0 + k < p.n) p.out[i0 + k] = at;
    at += c[k];
  }
  if (p.write_total && blockIdx.x == 0 && threadIdx.x == 0) p.out[p.n] = (uint32_t)p.tile_sums[p.ntiles];
}

}  // namespace

hipError_t launch_offsets_scan(const OffsetsScanParams& p, hipStream_t stream) {
  hipLaunchKernelGGL(scan_tile_sums_kernel, dim3((unsigned)p.ntiles), dim3(kScanBlock), 0, stream, p);
  hipLaunchKernelGGL(scan_totals_kernel, dim3(1), dim3(kScanBlock), 0, stream, p);
  hipLaunchKernelGGL(scan_offsets_kernel, dim3((unsigned)p.ntiles), dim3(kScanBlock), 0, stream, p);
  return hipGetLastError();
}

}  // namespace chq
