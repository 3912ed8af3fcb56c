// aggregate.hip -- the GROUP BY kernels (gfx950, wave64).  Host side: aggregate.cpp; the sort in front of them: sort.hip.
//
// The rows arrive ordered by the keys (`perm`), so a group is a run of consecutive sorted positions:
//   group heads      heads[i] = the keys of rows perm[i-1] and perm[i] differ (null-aware, by bits), heads per tile counted
//   head scan        tile counts -> exclusive scan (one workgroup) -> group id of every position, starts[g], rep[g]
//   segmented reduce one workgroup per tile of kAggTile positions: a thread reduces its kAggItems consecutive positions, a
//                    segmented scan over the threads (shuffles inside a wave, LDS between the waves) carries open runs across
//                    them; a group that lies inside the tile is written to out[g], the tile's share of a group that goes on
//                    into a neighbour tile to part_first / part_last
//   fold             one workgroup per tile boundary; the one that sits behind the FIRST tile of a group spanning several
//                    tiles combines that group's partials in tile order, by a tree whose shape depends on the tile count only
//   distinct         COUNT(DISTINCT c): the rows are sorted a second time, by (keys, c), and their runs found again (the FINE
//                    runs); a thread per group counts the fine runs between the group's two ends by binary search
// Every hand-off happens at a launch boundary: no workgroup waits for another, nothing spins, nothing depends on dispatch
// order.  No float atomics: a float sum is combined in an order fixed by the sorted positions, bit-identical from run to run.
#include <hip/hip_runtime.h>

#include "aggregate_acc.h"
#include "aggregate_device.h"

namespace chq {
namespace {

constexpr int kWaves = kScanWaves;
static_assert(kAggBlock == kScanBlock && kAggItems == kScanItems && kAggTile == kScanTile, "the aggregate's tiles (the join's and the window's too) are the shared scan geometry");

// ---- group heads ----------------------------------------------------------------------------------------------------------
// do rows a and b fall into different groups by this key?  (both null: the same group; else equal bit patterns)
__device__ __forceinline__ bool key_differs(const AggKey& k, uint32_t a, uint32_t b) {
  const bool va = !k.validity || bit_at(k.validity, k.bit_offset + a);
  const bool vb = !k.validity || bit_at(k.validity, k.bit_offset + b);
  if (va != vb) return true;
  if (!va) return false;
  switch (k.kind) {
    case AK_BOOL: return bit_at(k.values, k.bit_offset + a) != bit_at(k.values, k.bit_offset + b);
    case AK_UTF8: {
      const int32_t* offs = (const int32_t*)k.values;
      const int64_t sa = offs[a], sb = offs[b], la = offs[a + 1] - sa, lb = offs[b + 1] - sb;
      if (la != lb) return true;
      if (!k.data) return false;
      for (int64_t i = 0; i < la; ++i)
        if (k.data[sa + i] != k.data[sb + i]) return true;
      return false;
    }
    default:
      if (k.width == 16) {
        const uint64_t* v = (const uint64_t*)k.values;
        return v[2 * (uint64_t)a] != v[2 * (uint64_t)b] || v[2 * (uint64_t)a + 1] != v[2 * (uint64_t)b + 1];
      }
      return load_uint(k.values, a, k.width) != load_uint(k.values, b, k.width);
  }
}

// a thread owns kAggItems consecutive positions and stores their head bytes as one 8-byte word
static_assert(kAggItems == 8, "one u64 of head bytes per thread");
__global__ __launch_bounds__(kAggBlock) void agg_heads_kernel(const AggHeadsParams p) {
  __shared__ uint32_t sums[kWaves];
  const int64_t p0 = (int64_t)blockIdx.x * kAggTile + (int64_t)threadIdx.x * kAggItems;
  uint32_t row[kAggItems + 1];   // rows of positions p0 - 1 .. p0 + 7
#pragma unroll
  for (int k = 0; k <= kAggItems; ++k) {
    const int64_t pos = p0 - 1 + k;
    row[k] = pos >= 0 && pos < p.n ? (p.perm ? p.perm[pos] : (uint32_t)pos) : 0u;
  }
  uint64_t word = 0;
#pragma unroll
  for (int k = 0; k < kAggItems; ++k) {
    const int64_t pos = p0 + k;
    if (pos >= p.n) continue;
    bool head = pos == 0;
    for (int q = 0; q < p.n_keys && !head; ++q) head = key_differs(p.keys[q], row[k], row[k + 1]);
    word |= (uint64_t)(head ? 1 : 0) << (8 * k);
  }
  uint64_t* slot = (uint64_t*)(p.heads + p0);
  if (p.accumulate) word |= *slot;
  *slot = word;
  const uint32_t tot = block_sum<uint32_t>((uint32_t)__popcll(word), sums);
  if (threadIdx.x == 0) p.tile_counts[blockIdx.x] = tot;
}

// one workgroup: exclusive scan of the tile counts in place, the number of groups behind them
__global__ __launch_bounds__(kAggBlock) void agg_head_scan_kernel(const AggGroupsParams p) {
  __shared__ uint32_t sums[kWaves];
  scan_totals_in_place<uint32_t>(p.tile_counts, p.ntiles, p.tile_counts + p.ntiles, sums);
}

__global__ __launch_bounds__(kAggBlock) void agg_head_write_kernel(const AggGroupsParams p) {
  __shared__ uint32_t sums[kWaves];
  const int64_t p0 = (int64_t)blockIdx.x * kAggTile + (int64_t)threadIdx.x * kAggItems;
  const uint64_t word = *(const uint64_t*)(p.heads + p0);
  uint32_t tot;
  uint32_t g = block_exclusive_scan<uint32_t>((uint32_t)__popcll(word), sums, &tot) + p.tile_counts[blockIdx.x];   // heads before p0
#pragma unroll
  for (int k = 0; k < kAggItems; ++k) {
    const int64_t pos = p0 + k;
    if (pos >= p.n) continue;
    const bool head = (word >> (8 * k)) & 1;
    if (head) ++g;
    const uint32_t gid = g - 1;   // (position 0 is a head: g >= 1)
    p.gids[pos] = gid;
    if (head && (int64_t)gid < p.G) {
      p.starts[gid] = (uint32_t)pos;
      p.rep[gid] = p.perm ? p.perm[pos] : (uint32_t)pos;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) p.starts[p.G] = (uint32_t)p.n;
}

// ---- segmented reduce -------------------------------------------------------------------------------------------------------
// The run of group g inside tile `tile` is finished.  The group lies inside the tile: its value.  It began earlier: the
// tile's first run.  It goes on: the tile's last run.  (Began earlier AND goes on: the tile's only run, kept as its first.)
template <int OP>
__device__ __forceinline__ void agg_emit(const AggReduceParams& p, int64_t tile, uint32_t g, const AggAcc& acc) {
  const int64_t tbase = tile * kAggTile;
  const int64_t lo = p.starts[g], hi = p.starts[g + 1];
  if (lo < tbase) p.part_first[tile] = acc;
  else if (hi > tbase + kAggTile) p.part_last[tile] = acc;
  else acc_finalize<OP>(p, g, acc);
}

template <int OP>
__global__ __launch_bounds__(kAggBlock) void agg_reduce_kernel(const AggReduceParams p) {
  __shared__ AggAcc wave_acc[kWaves];
  __shared__ int wave_flag[kWaves];
  const int64_t tile = blockIdx.x;
  const int64_t tbase = tile * kAggTile;
  const int64_t tend = p.n - tbase < kAggTile ? p.n : tbase + kAggTile;
  const int64_t p0 = tbase + (int64_t)threadIdx.x * kAggItems;
  const bool has_items = p0 < tend;
  const int64_t next = p0 + kAggItems < tend ? p0 + kAggItems : tend;   // the position behind this thread's items

  // the thread's positions in order.  `run`: the run that is open at the current position; `any_head`: a run began inside
  // the thread.  A run that began before the thread and ends inside it waits in `first_acc` for what the earlier threads
  // hold of it; a run that begins and ends inside the thread is complete.
  AggAcc run = acc_identity<OP>(), first_acc = acc_identity<OP>();
  bool any_head = false, first_closed = false, ends_here = false;
  uint32_t first_gid = 0, last_gid = 0;
  if (has_items) {
    const uint32_t before = p0 > tbase ? p.gids[p0 - 1] : 0u;
#pragma unroll
    for (int k = 0; k < kAggItems; ++k) {
      const int64_t pos = p0 + k;
      if (pos >= tend) continue;
      const uint32_t g = p.gids[pos];
      const bool head = k == 0 ? (p0 == tbase || g != before) : g != last_gid;   // (the tile's first position opens a run)
      if (head && k > 0) {
        if (!any_head) { first_closed = true; first_acc = run; first_gid = last_gid; }
        else agg_emit<OP>(p, tile, last_gid, run);
        run = acc_identity<OP>();
      }
      any_head |= head;
      run = acc_combine<OP>(run, acc_load<OP>(p, pos));
      last_gid = g;
    }
    ends_here = next == tend || p.gids[next] != last_gid;
  }

  // segmented inclusive scan of (any_head, run) over the threads: (f1, v1) o (f2, v2) = (f1 | f2, f2 ? v2 : v1 + v2)
  const int lane = lane_id(), w = (int)(threadIdx.x >> 6);
  AggAcc x = run;
  int f = any_head ? 1 : 0;
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
  // what the earlier threads hold of the run that is open where this thread begins
  AggAcc carry = shfl_up_acc(x, 1);
  int fc = __shfl_up(f, 1u, 64);
  if (lane == 0) { carry = acc_identity<OP>(); fc = 0; }
  if (!fc) {
    AggAcc pre = acc_identity<OP>();
#pragma unroll
    for (int k = 0; k < kWaves; ++k)
      if (k < w) pre = wave_flag[k] ? wave_acc[k] : acc_combine<OP>(pre, wave_acc[k]);
    carry = acc_combine<OP>(pre, carry);
  }
  if (!has_items) return;
  if (first_closed) agg_emit<OP>(p, tile, first_gid, acc_combine<OP>(carry, first_acc));
  if (ends_here) agg_emit<OP>(p, tile, last_gid, any_head ? run : acc_combine<OP>(carry, run));
}

// Workgroup b - 1 looks at the boundary between tiles b - 1 and b.  When a group that BEGINS in tile b - 1 crosses it, the
// workgroup folds that group's partials -- part_last of tile b - 1, then part_first of every later tile the group reaches --
// in tile order: every thread a contiguous share, the threads by a fixed tree.
template <int OP>
__global__ __launch_bounds__(kAggBlock) void agg_fold_kernel(const AggReduceParams p) {
  __shared__ AggAcc wave_acc[kWaves];
  const int64_t b = (int64_t)blockIdx.x + 1;
  const int64_t bpos = b * kAggTile;
  if (bpos >= p.n) return;
  const uint32_t g = p.gids[bpos];
  const int64_t lo = p.starts[g], hi = p.starts[g + 1];
  const int64_t t0 = lo / kAggTile, t1 = (hi - 1) / kAggTile;
  if (lo >= bpos || t0 != b - 1) return;   // no group crosses here, or an earlier boundary's workgroup folds it
  const int64_t m = t1 - t0 + 1;
  const int64_t share = (m + kAggBlock - 1) / kAggBlock;
  const int64_t j0 = (int64_t)threadIdx.x * share, j1 = j0 + share < m ? j0 + share : m;
  AggAcc x = acc_identity<OP>();
  for (int64_t j = j0; j < j1; ++j) x = acc_combine<OP>(x, j == 0 ? p.part_last[t0] : p.part_first[t0 + j]);
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) x = acc_combine<OP>(x, shfl_down_acc(x, o));   // lane 0: lanes 0..63 in order
  if (lane_id() == 0) wave_acc[threadIdx.x >> 6] = x;
  __syncthreads();
  if (threadIdx.x == 0) {
    AggAcc tot = wave_acc[0];
#pragma unroll
    for (int k = 1; k < kWaves; ++k) tot = acc_combine<OP>(tot, wave_acc[k]);
    acc_finalize<OP>(p, g, tot);
  }
}

__global__ __launch_bounds__(kAggBlock) void agg_count_star_kernel(const AggCountStarParams p) {
  const int64_t g = (int64_t)blockIdx.x * kAggBlock + threadIdx.x;
  if (g < p.G) p.out[g] = (int64_t)p.starts[g + 1] - (int64_t)p.starts[g];
}

// COUNT(DISTINCT c): one group per thread.  Both ends of a group are starts of fine runs, so the two binary searches over
// starts2 find them exactly; the group's last fine run holds the nulls of c, if it has any (nulls sort last).
__device__ __forceinline__ int64_t fine_run_at(const AggDistinctParams& p, uint32_t pos) {
  int64_t lo = 0, hi = p.G2;   // the first index in [0, G2] whose start is >= pos (starts2[G2] = n >= pos)
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (p.starts2[mid] < pos) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}
__global__ __launch_bounds__(kAggBlock) void agg_distinct_kernel(const AggDistinctParams p) {
  const int64_t g = (int64_t)blockIdx.x * kAggBlock + threadIdx.x;
  if (g >= p.G) return;
  const int64_t lo = fine_run_at(p, p.starts[g]), hi = fine_run_at(p, p.starts[g + 1]);
  int64_t runs = hi - lo;
  if (runs > 0 && p.validity && !bit_at(p.validity, p.bit_offset + p.rep2[hi - 1])) --runs;
  p.out[g] = runs;
}

// one validity word of 32 groups per thread
__global__ __launch_bounds__(kAggBlock) void agg_validity_kernel(const AggValidityParams p) {
  const int64_t wi = (int64_t)blockIdx.x * kAggBlock + threadIdx.x;
  uint32_t word = 0;
  if (wi * 32 < p.G) {
    const int64_t g0 = wi * 32;
    const int n = p.G - g0 < 32 ? (int)(p.G - g0) : 32;
    for (int b = 0; b < n; ++b) word |= (uint32_t)(p.cnt[g0 + b] != 0) << b;
    ((uint32_t*)p.out)[wi] = word;
  }
  uint64_t ones = (uint64_t)__popc(word);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ones += __shfl_xor(ones, o, 64);
  if (lane_id() == 0 && ones) atomicAdd((unsigned long long*)p.ones, (unsigned long long)ones);
}

unsigned blocks_for(int64_t n, int64_t per) { return (unsigned)((n + per - 1) / per); }

template <int OP>
void launch_reduce(const AggReduceParams& p, hipStream_t stream) {
  hipLaunchKernelGGL(agg_reduce_kernel<OP>, dim3((unsigned)p.ntiles), dim3(kAggBlock), 0, stream, p);
  if (p.ntiles > 1) hipLaunchKernelGGL(agg_fold_kernel<OP>, dim3((unsigned)(p.ntiles - 1)), dim3(kAggBlock), 0, stream, p);
}

}  // namespace

hipError_t launch_agg_heads(const AggHeadsParams& p, hipStream_t stream) {
  hipLaunchKernelGGL(agg_heads_kernel, dim3((unsigned)p.ntiles), dim3(kAggBlock), 0, stream, p);
  return hipGetLastError();
}
hipError_t launch_agg_head_scan(const AggGroupsParams& p, hipStream_t stream) {
  hipLaunchKernelGGL(agg_head_scan_kernel, dim3(1), dim3(kAggBlock), 0, stream, p);
  return hipGetLastError();
}
hipError_t launch_agg_head_write(const AggGroupsParams& p, hipStream_t stream) {
  hipLaunchKernelGGL(agg_head_write_kernel, dim3((unsigned)p.ntiles), dim3(kAggBlock), 0, stream, p);
  return hipGetLastError();
}
hipError_t launch_agg_reduce(const AggReduceParams& p, hipStream_t stream) {
  switch (p.op) {
    case AO_COUNT: launch_reduce<AO_COUNT>(p, stream); break;
    case AO_SUM_INT: launch_reduce<AO_SUM_INT>(p, stream); break;
    case AO_SUM_FLOAT: launch_reduce<AO_SUM_FLOAT>(p, stream); break;
    case AO_MIN: launch_reduce<AO_MIN>(p, stream); break;
    case AO_MAX: launch_reduce<AO_MAX>(p, stream); break;
    case AO_AVG_INT: launch_reduce<AO_AVG_INT>(p, stream); break;
    case AO_AVG_FLOAT: launch_reduce<AO_AVG_FLOAT>(p, stream); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}
hipError_t launch_agg_distinct(const AggDistinctParams& p, hipStream_t stream) {
  hipLaunchKernelGGL(agg_distinct_kernel, dim3(blocks_for(p.G, kAggBlock)), dim3(kAggBlock), 0, stream, p);
  return hipGetLastError();
}
hipError_t launch_agg_count_star(const AggCountStarParams& p, hipStream_t stream) {
  hipLaunchKernelGGL(agg_count_star_kernel, dim3(blocks_for(p.G, kAggBlock)), dim3(kAggBlock), 0, stream, p);
  return hipGetLastError();
}
hipError_t launch_agg_validity(const AggValidityParams& p, hipStream_t stream) {
  hipLaunchKernelGGL(agg_validity_kernel, dim3(blocks_for(blocks_for(p.G, 32), kAggBlock)), dim3(kAggBlock), 0, stream, p);
  return hipGetLastError();
}

}  // namespace chq
