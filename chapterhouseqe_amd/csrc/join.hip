// join.hip -- the join kernels (gfx950, wave64): INNER, and what LEFT / FULL / LEFT_SEMI / LEFT_ANTI add to it.  Host side: join.cpp; in front of them: the sort (sort.hip) and the
// group heads of GROUP BY (aggregate.hip) over the concatenated keys, right rows first.
//
// A run of equal keys lies in the sorted positions as [right rows in input order][left rows in input order]:
//   split       split[g] = the position where the left rows of group g begin (a group with a null key: no right rows)
//   count       for every left row l: cnt[l] = right rows of its group, first[l] = their first position
//   scan        exclusive scan of cnt over the left rows in input order, the total in 64 bits: launch_offsets_scan (scan.hip)
//   expand      output j -> left row l = the largest l with off[l] <= j, right row perm[first[l] + (j - off[l])]: a binary
//               search per output, narrowed to the left rows the tile covers -- O(log nL) at worst whatever the skew, and
//               no thread walks a run or a gap
// The other kinds run the same split and scan and replace count and expand by their siblings:
//   count_kind  the count rule of the kind over c = cnt[l]: max(c, 1) (LEFT, FULL; an unmatched row: first[l] = "no row"),
//               c > 0 (SEMI), c == 0 (ANTI)
//   expand_kind as expand; a left row marked "no row" writes ridx[j] = "no row"; SEMI and ANTI write lidx only
//   tail        FULL: flag[r] = right row r lies in a run with a null key or without left rows (one pass over the sorted
//               positions), the same scan over the flags, then lidx[M_left + off[r]] = "no row", ridx[...] = r: one writer
//               per slot
// INNER launches exactly the kernels it launched before the other kinds existed.
// Every hand-off happens at a launch boundary: no workgroup waits for another, nothing spins, no atomics, nothing depends on
// dispatch order.  The result is bit-identical from run to run.
#include <hip/hip_runtime.h>

#include "join_device.h"
#include "scan_device.h"

namespace chq {
namespace {

// ---- split ------------------------------------------------------------------------------------------------------------------
// Exactly one position per group writes: the last right row of the group, or -- a group without right rows -- its head.
__global__ __launch_bounds__(kJoinBlock) void join_split_kernel(const JoinSplitParams p) {
  const int64_t p0 = (int64_t)blockIdx.x * kJoinTile + (int64_t)threadIdx.x * kJoinItems;
#pragma unroll
  for (int k = 0; k < kJoinItems; ++k) {
    const int64_t pos = p0 + k;
    if (pos >= p.n) continue;
    const uint32_t row = p.perm ? p.perm[pos] : (uint32_t)pos;
    const uint32_t g = p.gids[pos];
    bool writes;
    if ((int64_t)row < p.n_right) {
      writes = pos + 1 == p.n || p.gids[pos + 1] != g || (int64_t)(p.perm ? p.perm[pos + 1] : (uint32_t)(pos + 1)) >= p.n_right;
    } else {
      writes = pos == 0 || p.gids[pos - 1] != g;
    }
    if (!writes) continue;
    bool null_key = false;
    for (int q = 0; q < p.n_keys; ++q) null_key |= p.validity[q] && !bit_at(p.validity[q], p.bit_offset[q] + row);
    if (null_key) p.split[g] = p.starts[g];
    else if (!p.nulls_only) p.split[g] = (int64_t)row < p.n_right ? (uint32_t)(pos + 1) : p.starts[g];
  }
}

// ---- count ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kJoinBlock) void join_count_kernel(const JoinCountParams p) {
  const int64_t p0 = (int64_t)blockIdx.x * kJoinTile + (int64_t)threadIdx.x * kJoinItems;
#pragma unroll
  for (int k = 0; k < kJoinItems; ++k) {
    const int64_t pos = p0 + k;
    if (pos >= p.n) continue;
    const uint32_t row = p.perm ? p.perm[pos] : (uint32_t)pos;
    if ((int64_t)row < p.n_right) continue;
    const uint32_t l = row - (uint32_t)p.n_right;
    const uint32_t g = p.gids[pos];
    const uint32_t s = p.starts[g];
    p.cnt[l] = p.split[g] - s;
    p.first[l] = s;
  }
}

// the same pass with the count rule of an outer, semi or anti join
__global__ __launch_bounds__(kJoinBlock) void join_count_kind_kernel(const JoinCountKindParams q) {
  const JoinCountParams& p = q.base;
  const int64_t p0 = (int64_t)blockIdx.x * kJoinTile + (int64_t)threadIdx.x * kJoinItems;
#pragma unroll
  for (int k = 0; k < kJoinItems; ++k) {
    const int64_t pos = p0 + k;
    if (pos >= p.n) continue;
    const uint32_t row = p.perm ? p.perm[pos] : (uint32_t)pos;
    if ((int64_t)row < p.n_right) continue;
    const uint32_t l = row - (uint32_t)p.n_right;
    const uint32_t g = p.gids[pos];
    const uint32_t s = p.starts[g];
    const uint32_t c = p.split[g] - s;
    if (q.rule == JOIN_COUNT_PADDED) {
      p.cnt[l] = c ? c : 1u;
      p.first[l] = c ? s : kJoinNoRow;
    } else {
      p.cnt[l] = q.rule == JOIN_COUNT_SEMI ? (c != 0) : (c == 0);
    }
  }
}

// ---- expand -----------------------------------------------------------------------------------------------------------------
// the largest l in [lo, hi] with off[l] <= j (off is non-decreasing, off[lo] <= j)
__device__ __forceinline__ int64_t last_at_most(const uint32_t* off, int64_t lo, int64_t hi, uint32_t j) {
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo + 1) / 2;
    if (off[mid] <= j) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(kJoinBlock) void join_expand_kernel(const JoinExpandParams p) {
  __shared__ int64_t bounds[2];
  const int64_t j0 = (int64_t)blockIdx.x * kJoinTile;
  const int64_t j1 = p.m - j0 < kJoinTile ? p.m : j0 + kJoinTile;   // (j0 < m: the grid covers [0, m))
  // the left rows of the tile's first and last output bound every search of the tile
  if (threadIdx.x < 2) bounds[threadIdx.x] = last_at_most(p.off, 0, p.n_left - 1, (uint32_t)(threadIdx.x ? j1 - 1 : j0));
  __syncthreads();
  const int64_t lo = bounds[0], hi = bounds[1];
#pragma unroll
  for (int k = 0; k < kJoinItems; ++k) {
    const int64_t j = j0 + (int64_t)k * kJoinBlock + threadIdx.x;   // consecutive lanes, consecutive outputs
    if (j >= j1) continue;
    const int64_t l = last_at_most(p.off, lo, hi, (uint32_t)j);
    const int64_t pos = (int64_t)p.first[l] + (j - (int64_t)p.off[l]);
    p.lidx[j] = (uint32_t)l;
    p.ridx[j] = p.perm ? p.perm[pos] : (uint32_t)pos;
  }
}

// kRight: the kinds with right rows (LEFT, FULL); else SEMI and ANTI, whose counts are 0 or 1
template <bool kRight>
__global__ __launch_bounds__(kJoinBlock) void join_expand_kind_kernel(const JoinExpandParams p) {
  __shared__ int64_t bounds[2];
  const int64_t j0 = (int64_t)blockIdx.x * kJoinTile;
  const int64_t j1 = p.m - j0 < kJoinTile ? p.m : j0 + kJoinTile;
  if (threadIdx.x < 2) bounds[threadIdx.x] = last_at_most(p.off, 0, p.n_left - 1, (uint32_t)(threadIdx.x ? j1 - 1 : j0));
  __syncthreads();
  const int64_t lo = bounds[0], hi = bounds[1];
#pragma unroll
  for (int k = 0; k < kJoinItems; ++k) {
    const int64_t j = j0 + (int64_t)k * kJoinBlock + threadIdx.x;
    if (j >= j1) continue;
    const int64_t l = last_at_most(p.off, lo, hi, (uint32_t)j);
    p.lidx[j] = (uint32_t)l;
    if constexpr (kRight) {
      const uint32_t f = p.first[l];
      uint32_t r = kJoinNoRow;
      if (f != kJoinNoRow) {
        const int64_t pos = (int64_t)f + (j - (int64_t)p.off[l]);
        r = p.perm ? p.perm[pos] : (uint32_t)pos;
      }
      p.ridx[j] = r;
    }
  }
}

// ---- FULL's tail ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kJoinBlock) void join_tail_flag_kernel(const JoinTailParams p) {
  const int64_t p0 = (int64_t)blockIdx.x * kJoinTile + (int64_t)threadIdx.x * kJoinItems;
#pragma unroll
  for (int k = 0; k < kJoinItems; ++k) {
    const int64_t pos = p0 + k;
    if (pos >= p.n) continue;
    const uint32_t row = p.perm ? p.perm[pos] : (uint32_t)pos;
    if ((int64_t)row >= p.n_right) continue;
    const uint32_t g = p.gids[pos];
    const uint32_t sp = p.split[g];
    p.flag[row] = sp == p.starts[g] || sp == p.starts[g + 1];
  }
}

__global__ __launch_bounds__(kJoinBlock) void join_tail_write_kernel(const JoinTailParams p) {
  const int64_t r0 = (int64_t)blockIdx.x * kJoinTile + (int64_t)threadIdx.x * kJoinItems;
#pragma unroll
  for (int k = 0; k < kJoinItems; ++k) {
    const int64_t r = r0 + k;
    if (r >= p.n_right || !p.flag[r]) continue;
    const int64_t j = p.m_left + (int64_t)p.off[r];
    if (j >= p.m) continue;   // (never taken: off[r] < the tail's length)
    p.lidx[j] = kJoinNoRow;
    p.ridx[j] = (uint32_t)r;
  }
}

unsigned tiles_of(int64_t n) { return (unsigned)((n + kJoinTile - 1) / kJoinTile); }

}  // namespace

hipError_t launch_join_split(const JoinSplitParams& p, hipStream_t stream) {
  hipLaunchKernelGGL(join_split_kernel, dim3(tiles_of(p.n)), dim3(kJoinBlock), 0, stream, p);
  return hipGetLastError();
}
hipError_t launch_join_count(const JoinCountParams& p, hipStream_t stream) {
  hipLaunchKernelGGL(join_count_kernel, dim3(tiles_of(p.n)), dim3(kJoinBlock), 0, stream, p);
  return hipGetLastError();
}
hipError_t launch_join_count_kind(const JoinCountKindParams& p, hipStream_t stream) {
  hipLaunchKernelGGL(join_count_kind_kernel, dim3(tiles_of(p.base.n)), dim3(kJoinBlock), 0, stream, p);
  return hipGetLastError();
}
hipError_t launch_join_expand(const JoinExpandParams& p, hipStream_t stream) {
  hipLaunchKernelGGL(join_expand_kernel, dim3(tiles_of(p.m)), dim3(kJoinBlock), 0, stream, p);
  return hipGetLastError();
}
hipError_t launch_join_expand_kind(const JoinExpandParams& p, bool right, hipStream_t stream) {
  if (right) hipLaunchKernelGGL(join_expand_kind_kernel<true>, dim3(tiles_of(p.m)), dim3(kJoinBlock), 0, stream, p);
  else hipLaunchKernelGGL(join_expand_kind_kernel<false>, dim3(tiles_of(p.m)), dim3(kJoinBlock), 0, stream, p);
  return hipGetLastError();
}
hipError_t launch_join_tail_flag(const JoinTailParams& p, hipStream_t stream) {
  hipLaunchKernelGGL(join_tail_flag_kernel, dim3(tiles_of(p.n)), dim3(kJoinBlock), 0, stream, p);
  return hipGetLastError();
}
hipError_t launch_join_tail_write(const JoinTailParams& p, hipStream_t stream) {
  hipLaunchKernelGGL(join_tail_write_kernel, dim3(tiles_of(p.n_right)), dim3(kJoinBlock), 0, stream, p);
  return hipGetLastError();
}

}  // namespace chq
