// window.hip -- the window-function kernels (gfx950, wave64).  Host side: window.cpp; the sort and the run finder in front
// of them: sort.hip, aggregate.hip (group heads, head scan, head write).
//
// The rows arrive ordered by the partition keys, then the order keys (`perm`); pgid / pstarts describe the partitions and
// qgid / qstarts the peer groups as runs of sorted positions.
//   rank             row_number, rank and dense_rank of every position from the run starts alone
//   shift            the row id `offset` positions before / behind, or "no row" outside the partition: LAG / LEAD are then
//                    the null-producing gather of the outer joins
//   segmented scan   win_scan_kernel: one workgroup per tile of kWinTile positions scans its tile (a thread its kWinItems
//                    consecutive positions, shuffles inside a wave, LDS between the waves) and leaves the total of the run
//                    that is open at the tile's end; win_carry_kernel: ONE workgroup scans those totals over the tiles;
//                    win_emit_kernel: every position picks the scanned element its frame ends at, adds the carry of that
//                    element's tile when the partition began before the tile, converts it and writes it to the row
// Every hand-off happens at a launch boundary: no workgroup waits for another, nothing spins, nothing depends on dispatch
// order.  No float atomics: a float sum is combined in an order fixed by the sorted positions, bit-identical from run to run.
// The accumulator (identity, combine, load, conversion) is GROUP BY's: aggregate_acc.h.
#include <hip/hip_runtime.h>

#include "aggregate_acc.h"
#include "sort_device.h"
#include "window_device.h"

namespace chq {
namespace {

constexpr int kWaves = kWinBlock / 64;

// Segmented inclusive scan of (f, x) over the workgroup's threads: (f1, v1) o (f2, v2) = (f1 | f2, f2 ? v2 : v1 + v2).
// `before` stands in front of thread 0 (with no flag).  Returns what stands in front of THIS thread -- the combination of
// every earlier thread back to the last flag, `before` included when no earlier thread has a flag -- and leaves the
// thread's own inclusive result in x / f.
template <int OP>
__device__ __forceinline__ AggAcc block_segmented_scan(AggAcc& x, int& f, const AggAcc& before, AggAcc* wave_acc, int* wave_flag) {
  const int lane = lane_id(), w = (int)(threadIdx.x >> 6);
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const AggAcc y = shfl_up_acc(x, o);
    const int fy = __shfl_up(f, (unsigned)o, 64);
    if (lane >= o) {
      if (!f) x = acc_combine<OP>(y, x);
      f |= fy;
    }
  }
  if (lane == 63) { wave_acc[w] = x; wave_flag[w] = f; }
  __syncthreads();
  AggAcc pre = before;   // the earlier waves, back to their last flag
#pragma unroll
  for (int k = 0; k < kWaves; ++k)
    if (k < w) pre = wave_flag[k] ? wave_acc[k] : acc_combine<OP>(pre, wave_acc[k]);
  AggAcc carry = shfl_up_acc(x, 1);
  int fc = __shfl_up(f, 1u, 64);
  if (lane == 0) { carry = pre; fc = 1; }
  if (!fc) carry = acc_combine<OP>(pre, carry);
  if (!f) x = acc_combine<OP>(pre, x);
  __syncthreads();   // wave_acc / wave_flag may be reused
  return carry;
}

// ---- ranks ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kWinBlock) void win_rank_kernel(const WinRankParams p) {
  const int64_t tbase = (int64_t)blockIdx.x * kWinTile;
#pragma unroll
  for (int k = 0; k < kWinItems; ++k) {
    const int64_t i = tbase + (int64_t)k * kWinBlock + threadIdx.x;
    if (i >= p.n) continue;
    const uint32_t row = p.perm ? p.perm[i] : (uint32_t)i;
    const uint32_t ps = p.pstarts[p.pgid[i]];
    if (p.row_number) p.row_number[row] = i - (int64_t)ps + 1;
    if (p.rank || p.dense_rank) {
      const uint32_t q = p.qgid[i];
      if (p.rank) p.rank[row] = (int64_t)p.qstarts[q] - (int64_t)ps + 1;
      if (p.dense_rank) p.dense_rank[row] = (int64_t)q - (int64_t)p.qgid[ps] + 1;
    }
  }
}

// ---- LAG / LEAD -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kWinBlock) void win_shift_kernel(const WinShiftParams p) {
  const int64_t tbase = (int64_t)blockIdx.x * kWinTile;
#pragma unroll
  for (int k = 0; k < kWinItems; ++k) {
    const int64_t i = tbase + (int64_t)k * kWinBlock + threadIdx.x;
    if (i >= p.n) continue;
    const uint32_t g = p.pgid[i];
    const int64_t j = i + p.delta;
    uint32_t src = kSortNoRow;
    if (j >= (int64_t)p.pstarts[g] && j < (int64_t)p.pstarts[g + 1]) src = p.perm ? p.perm[j] : (uint32_t)j;
    p.src[p.perm ? p.perm[i] : (uint32_t)i] = src;
  }
}

// ---- segmented scan -------------------------------------------------------------------------------------------------------
template <int OP>
__device__ __forceinline__ void scan_store(const WinAggParams& p, int64_t pos, const AggAcc& x) {
  if (OP != AO_COUNT) p.scan_a[pos] = x.a;
  if (OP == AO_SUM_INT) p.scan_b[pos] = x.b;
  p.scan_cnt[pos] = (uint32_t)x.cnt;
}
template <int OP>
__device__ __forceinline__ AggAcc scan_load(const WinAggParams& p, int64_t pos) {
  AggAcc x{0, 0, 0};
  if (OP != AO_COUNT) x.a = p.scan_a[pos];
  if (OP == AO_SUM_INT) x.b = p.scan_b[pos];
  x.cnt = p.scan_cnt[pos];
  return x;
}

// The scan of one tile, as if the tile stood alone: element i = the combination of the values from max(the start of i's
// partition, the tile's first position) through i.  A thread scans its kWinItems consecutive positions; what the earlier
// threads hold of the run that is open where the thread begins reaches it through the segmented scan over the threads.
static_assert(kWinItems == 8, "eight positions per thread");
template <int OP>
__global__ __launch_bounds__(kWinBlock) void win_scan_kernel(const WinAggParams p) {
  __shared__ AggAcc wave_acc[kWaves];
  __shared__ int wave_flag[kWaves];
  const int64_t tile = blockIdx.x;
  const int64_t tbase = tile * kWinTile;
  const int64_t tend = p.n - tbase < kWinTile ? p.n : tbase + kWinTile;
  const int64_t p0 = tbase + (int64_t)threadIdx.x * kWinItems;

  AggAcc loc[kWinItems];
  AggAcc run = acc_identity<OP>();
  int first_head = kWinItems;   // the thread's first position that begins a partition (none: kWinItems)
  if (p0 < tend) {
    uint32_t prev = p.pgid[p0 > tbase ? p0 - 1 : p0];   // (the tile's first position needs no reset: nothing stands before it)
#pragma unroll
    for (int k = 0; k < kWinItems; ++k) {
      const int64_t pos = p0 + k;
      if (pos >= tend) { loc[k] = run; continue; }
      const uint32_t g = p.pgid[pos];
      if (g != prev) {
        run = acc_identity<OP>();
        if (first_head == kWinItems) first_head = k;
      }
      run = acc_combine<OP>(run, acc_load<OP>(p, pos));
      loc[k] = run;
      prev = g;
    }
  }
  AggAcc x = run;
  int f = first_head < kWinItems ? 1 : 0;
  const AggAcc carry = block_segmented_scan<OP>(x, f, acc_identity<OP>(), wave_acc, wave_flag);
  if (p0 >= tend) return;
#pragma unroll
  for (int k = 0; k < kWinItems; ++k) {
    const int64_t pos = p0 + k;
    if (pos >= tend) continue;
    const AggAcc v = k < first_head ? acc_combine<OP>(carry, loc[k]) : loc[k];
    scan_store<OP>(p, pos, v);
    if (pos == tend - 1) p.tile_tot[tile] = v;
  }
}

// One workgroup: the segmented inclusive scan of the tile totals, kWinCarryRound tiles a round.  A tile's total restarts
// the scan when the run it belongs to began inside the tile.
template <int OP>
__global__ __launch_bounds__(kWinBlock) void win_carry_kernel(const WinAggParams p) {
  __shared__ AggAcc wave_acc[kWaves];
  __shared__ int wave_flag[kWaves];
  __shared__ AggAcc round_acc;
  AggAcc before = acc_identity<OP>();   // the scan at the last tile of the earlier rounds
  for (int64_t c0 = 0; c0 < p.ntiles; c0 += kWinCarryRound) {
    const int64_t t = c0 + threadIdx.x;
    AggAcc x = acc_identity<OP>();
    int f = 0;
    if (t < p.ntiles) {
      const int64_t tbase = t * kWinTile;
      const int64_t tend = p.n - tbase < kWinTile ? p.n : tbase + kWinTile;
      x = p.tile_tot[t];
      f = (int64_t)p.pstarts[p.pgid[tend - 1]] >= tbase ? 1 : 0;
    }
    block_segmented_scan<OP>(x, f, before, wave_acc, wave_flag);
    if (t < p.ntiles) p.tile_carry[t] = x;
    if (threadIdx.x == kWinBlock - 1) round_acc = x;
    __syncthreads();
    before = round_acc;
    __syncthreads();
  }
}

// Every position reads the scanned element its frame ends at; that element may lie in a later tile than the position.
template <int OP>
__global__ __launch_bounds__(kWinBlock) void win_emit_kernel(const WinAggParams p) {
  const int64_t tbase = (int64_t)blockIdx.x * kWinTile;
#pragma unroll
  for (int k = 0; k < kWinItems; ++k) {
    const int64_t i = tbase + (int64_t)k * kWinBlock + threadIdx.x;
    if (i >= p.n) continue;
    const uint32_t g = p.pgid[i];
    const int64_t ps = p.pstarts[g];
    int64_t j = i;
    if (p.frame == WF_RANGE) j = (int64_t)p.qstarts[p.qgid[i] + 1] - 1;
    else if (p.frame == WF_PARTITION) j = (int64_t)p.pstarts[g + 1] - 1;
    AggAcc acc{0, 0, (uint64_t)(j - ps + 1)};   // no scan: the rows of the frame
    if (p.scan_cnt) {
      acc = scan_load<OP>(p, j);
      const int64_t tj = j / kWinTile;
      if (ps < tj * kWinTile) acc = acc_combine<OP>(p.tile_carry[tj - 1], acc);
    }
    acc_finalize<OP>(p, p.perm ? p.perm[i] : (uint32_t)i, acc);
  }
}

unsigned tiles_of(int64_t n) { return (unsigned)((n + kWinTile - 1) / kWinTile); }

template <int OP>
void launch_scan(const WinAggParams& p, hipStream_t stream) {
  hipLaunchKernelGGL(win_scan_kernel<OP>, dim3((unsigned)p.ntiles), dim3(kWinBlock), 0, stream, p);
  hipLaunchKernelGGL(win_carry_kernel<OP>, dim3(1), dim3(kWinBlock), 0, stream, p);
}
template <int OP>
void launch_emit(const WinAggParams& p, hipStream_t stream) {
  hipLaunchKernelGGL(win_emit_kernel<OP>, dim3((unsigned)p.ntiles), dim3(kWinBlock), 0, stream, p);
}

}  // namespace

hipError_t launch_win_rank(const WinRankParams& p, hipStream_t stream) {
  hipLaunchKernelGGL(win_rank_kernel, dim3(tiles_of(p.n)), dim3(kWinBlock), 0, stream, p);
  return hipGetLastError();
}
hipError_t launch_win_shift(const WinShiftParams& p, hipStream_t stream) {
  hipLaunchKernelGGL(win_shift_kernel, dim3(tiles_of(p.n)), dim3(kWinBlock), 0, stream, p);
  return hipGetLastError();
}
hipError_t launch_win_scan(const WinAggParams& p, hipStream_t stream) {
  switch (p.op) {
    case AO_COUNT: launch_scan<AO_COUNT>(p, stream); break;
    case AO_SUM_INT: launch_scan<AO_SUM_INT>(p, stream); break;
    case AO_SUM_FLOAT: launch_scan<AO_SUM_FLOAT>(p, stream); break;
    case AO_MIN: launch_scan<AO_MIN>(p, stream); break;
    case AO_MAX: launch_scan<AO_MAX>(p, stream); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}
hipError_t launch_win_emit(const WinAggParams& p, hipStream_t stream) {
  switch (p.op) {
    case AO_COUNT: launch_emit<AO_COUNT>(p, stream); break;
    case AO_SUM_INT: launch_emit<AO_SUM_INT>(p, stream); break;
    case AO_SUM_FLOAT: launch_emit<AO_SUM_FLOAT>(p, stream); break;
    case AO_MIN: launch_emit<AO_MIN>(p, stream); break;
    case AO_MAX: launch_emit<AO_MAX>(p, stream); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace chq
