// partition.hip -- the hash partitioning kernels (gfx950, wave64): the pinned row hash over the key columns, the per-tile
// counts of every partition, their scan and the scatter of the row ids.  Host side: partition.cpp.
//
// The structure is one radix pass of sort.hip with the partition id as the digit: three launches that hand data over only
// at launch boundaries (hash + count -> scan -> scatter).  No workgroup waits on another inside a launch, nothing spins and
// nothing depends on dispatch order; the only atomics are integer adds, whose result does not depend on their order.
#include <hip/hip_runtime.h>

#include "partition_device.h"
#include "scan_device.h"

namespace chq {
namespace {

constexpr int kWaves = kScanWaves;
static_assert(kPartBlock == kScanBlock && kPartItems == kScanItems && kPartTile == kScanTile, "the partitioning's tiles are the shared scan geometry");
static_assert(kPartBlock == kPartMaxPartitions, "one thread per partition id in the count, scan and scatter kernels");

// ---- the pinned hash (include/chq.h: chq_partition_records) ------------------------------------------------------------
constexpr uint64_t kGold = 0x9E3779B97F4A7C15ull;

__device__ __forceinline__ uint64_t fmix64(uint64_t x) {
  x ^= x >> 33; x *= 0xFF51AFD7ED558CCDull;
  x ^= x >> 33; x *= 0xC4CEB9FE1A85EC53ull;
  x ^= x >> 33;
  return x;
}

// V of row r of one key: 0 for a null, else fmix64 chained over the 8-byte little-endian chunks of the value's bytes
__device__ __forceinline__ uint64_t value_hash(const PartKey& k, uint32_t r) {
  if (k.validity && !bit_at(k.validity, k.bit_offset + r)) return 0;
  switch (k.kind) {
    case PK_BOOL: return fmix64(fmix64(2) ^ (bit_at(k.values, k.bit_offset + r) ? 1ull : 0ull));
    case PK_UTF8: {
      const int32_t* offs = (const int32_t*)k.values;
      const int64_t start = offs[r], len = k.data ? (int64_t)offs[(int64_t)r + 1] - start : 0;
      uint64_t acc = fmix64((uint64_t)len + 1);
      const uint8_t* s = k.data + start;
      for (int64_t at = 0; at < len; at += 8) {
        const int take = len - at < 8 ? (int)(len - at) : 8;
        uint64_t chunk = 0;
        for (int b = 0; b < take; ++b) chunk |= (uint64_t)s[at + b] << (8 * b);
        acc = fmix64(acc ^ chunk);
      }
      return acc;
    }
    default: {
      uint64_t acc = fmix64((uint64_t)k.width + 1);
      switch (k.width) {
        case 1: return fmix64(acc ^ k.values[r]);
        case 2: return fmix64(acc ^ ((const uint16_t*)k.values)[r]);
        case 4: return fmix64(acc ^ ((const uint32_t*)k.values)[r]);
        case 8: return fmix64(acc ^ ((const uint64_t*)k.values)[r]);
        default: {   // 16
          const uint64_t* v = (const uint64_t*)k.values + 2 * (uint64_t)r;
          acc = fmix64(acc ^ v[0]);
          return fmix64(acc ^ v[1]);
        }
      }
    }
  }
}

// ---- hash + count ----------------------------------------------------------------------------------------------------------
// Tile t = rows [t kPartTile, (t+1) kPartTile); wave w of its workgroup owns the w-th quarter, item j of lane l being row
// w * kPartTile/4 + j * 64 + l.  Both the count here and the scatter rank rows in that order, which is the input order: stable.
__global__ __launch_bounds__(kPartBlock) void part_hash_kernel(const PartHashParams p) {
  __shared__ uint32_t cnt[kPartMaxPartitions];
  cnt[threadIdx.x] = 0;
  __syncthreads();
  const int64_t tile = blockIdx.x;
  const int64_t wbase = tile * kPartTile + (int64_t)(threadIdx.x >> 6) * (kPartTile / kWaves);
  for (int j = 0; j < kPartItems; ++j) {
    const int64_t i = wbase + j * 64 + lane_id();
    const bool valid = i < p.n;
    uint64_t h = 0;
    if (valid) {
      h = p.first ? kGold : p.carry[i];
      for (int q = 0; q < p.n_keys; ++q) h = fmix64(h * kGold + value_hash(p.keys[q], (uint32_t)i));
    }
    if (!p.last) {   // (uniform: more keys follow in a further launch)
      if (valid) p.carry[i] = h;
      continue;
    }
    const uint32_t d = valid ? (uint32_t)(((h >> 32) * (uint64_t)p.n_partitions) >> 32) : 0u;
    if (valid) p.ids[i] = (uint8_t)d;
    const uint64_t peers = byte_peers(d, __ballot(valid));
    if (valid && (peers & lanes_below()) == 0) atomicAdd(&cnt[d], (uint32_t)__popcll(peers));
  }
  __syncthreads();
  if (p.last && threadIdx.x < p.n_partitions) {
    const uint32_t c = cnt[threadIdx.x];
    p.tile_counts[(int64_t)threadIdx.x * p.ntiles + tile] = c;
    if (c) atomicAdd(&p.totals[threadIdx.x], c);
  }
}

// workgroup d: exclusive scan of partition d's tile counts, offset by the rows of the smaller partitions
__global__ __launch_bounds__(kPartBlock) void part_scan_kernel(const PartScatterParams p) {
  __shared__ uint32_t sums[kWaves];
  const unsigned d = blockIdx.x;
  const uint32_t before = block_sum<uint32_t>(threadIdx.x < d ? p.totals[threadIdx.x] : 0u, sums);
  scan_count_rows<kPartItems>(p.tile_counts + (int64_t)d * p.ntiles, p.ntiles, before, sums);
}

// ranks every row of the tile, stages the row ids in LDS in partition order, then writes each partition's run contiguously
__global__ __launch_bounds__(kPartBlock) void part_scatter_kernel(const PartScatterParams p) {
  __shared__ uint32_t sv[kPartTile];
  __shared__ uint8_t sd[kPartTile];
  __shared__ uint32_t wcnt[kWaves][kPartMaxPartitions];
  __shared__ uint32_t dstart[kPartMaxPartitions];
  __shared__ uint32_t gbase[kPartMaxPartitions];
  __shared__ uint32_t sums[kWaves];
  const int w = (int)(threadIdx.x >> 6);
  for (int k = threadIdx.x; k < kWaves * kPartMaxPartitions; k += kPartBlock) (&wcnt[0][0])[k] = 0;
  const int64_t tile = blockIdx.x;
  const int64_t tbase = tile * kPartTile;
  const int64_t wbase = tbase + (int64_t)w * (kPartTile / kWaves);
  uint32_t id[kPartItems];
#pragma unroll
  for (int j = 0; j < kPartItems; ++j) {
    const int64_t i = wbase + j * 64 + lane_id();
    id[j] = i < p.n ? p.ids[i] : 0u;
  }
  __syncthreads();
  uint32_t pos[kPartItems];
  const uint32_t out0 = threadIdx.x < p.n_partitions ? p.tile_counts[(int64_t)threadIdx.x * p.ntiles + tile] : 0u;
  tile_positions<kPartItems>([&](int j) { return id[j]; }, wbase, p.n, wcnt, dstart, sums, pos);
  gbase[threadIdx.x] = out0 - dstart[threadIdx.x];   // (mod 2^32: gbase + position < 2^32)
#pragma unroll
  for (int j = 0; j < kPartItems; ++j) {
    const int64_t i = wbase + j * 64 + lane_id();
    if (i < p.n && pos[j] < (uint32_t)kPartTile) {
      sv[pos[j]] = (uint32_t)i;
      sd[pos[j]] = (uint8_t)id[j];
    }
  }
  __syncthreads();
  const int64_t left = p.n - tbase;
  const int tile_n = left < kPartTile ? (int)left : kPartTile;
  for (int q = threadIdx.x; q < tile_n; q += kPartBlock) {
    const uint32_t dst = gbase[sd[q]] + (uint32_t)q;
    if ((int64_t)dst >= p.n) continue;   // (never taken: the positions are a permutation of [0, n))
    p.perm[dst] = sv[q];
  }
}

}  // namespace

hipError_t launch_part_hash(const PartHashParams& p, hipStream_t stream) {
  hipLaunchKernelGGL(part_hash_kernel, dim3((unsigned)p.ntiles), dim3(kPartBlock), 0, stream, p);
  return hipGetLastError();
}
hipError_t launch_part_scatter(const PartScatterParams& p, hipStream_t stream) {
  hipLaunchKernelGGL(part_scan_kernel, dim3(p.n_partitions), dim3(kPartBlock), 0, stream, p);
  hipLaunchKernelGGL(part_scatter_kernel, dim3((unsigned)p.ntiles), dim3(kPartBlock), 0, stream, p);
  return hipGetLastError();
}

}  // namespace chq
