// scan_device.h -- device side only (.hip files include it): the one workgroup geometry of every tiled operator and the scan
// pieces they share -- the small loads, the workgroup sum and exclusive scan, the one-workgroup scan of tile totals in rounds,
// the scan of a row of per-tile counts, the bitmap words and row copies of the Parquet kernels, and the ranking of a tile's
// items by an 8-bit id (radix pass, hash partitioning).
// Everything here is integer arithmetic: the result does not depend on the order of the additions.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace chq {

constexpr int kScanBlock = 256;                      // threads of a workgroup
constexpr int kScanWaves = kScanBlock / 64;          // 4 waves
constexpr int kScanItems = 8;                        // items per thread
constexpr int kScanTile = kScanBlock * kScanItems;   // items per workgroup tile

__device__ __forceinline__ int lane_id() { return (int)(threadIdx.x & 63); }
__device__ __forceinline__ uint64_t lanes_below() { return (1ull << lane_id()) - 1; }
// the lanes below this one whose bit is set in m: two v_mbcnt, no mask to build (popcount(m & lanes_below()) costs a 64-bit
// shift, two ands, two counts and two more VGPRs)
__device__ __forceinline__ uint32_t lane_rank64(uint64_t m) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0));
}
__device__ __forceinline__ bool bit_at(const void* bits, int64_t pos) { return (((const uint8_t*)bits)[pos >> 3] >> (pos & 7)) & 1; }

__device__ __forceinline__ uint64_t load_uint(const uint8_t* values, uint32_t r, int width) {
  switch (width) {
    case 1: return values[r];
    case 2: return ((const uint16_t*)values)[r];
    case 4: return ((const uint32_t*)values)[r];
    default: return ((const uint64_t*)values)[r];
  }
}
__device__ __forceinline__ int64_t load_int(const uint8_t* values, uint32_t r, int width) {
  switch (width) {
    case 1: return ((const int8_t*)values)[r];
    case 2: return ((const int16_t*)values)[r];
    case 4: return ((const int32_t*)values)[r];
    default: return ((const int64_t*)values)[r];
  }
}

// sum of every thread's v over the workgroup; wave_sums: kScanWaves words of LDS
template <typename T>
__device__ __forceinline__ T block_sum(T v, T* wave_sums) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if (lane_id() == 0) wave_sums[threadIdx.x >> 6] = v;
  __syncthreads();
  T tot = 0;
#pragma unroll
  for (int k = 0; k < kScanWaves; ++k) tot += wave_sums[k];
  __syncthreads();   // wave_sums may be reused
  return tot;
}

// exclusive prefix of `v` over the workgroup (thread order); *total = sum of every thread's v
template <typename T>
__device__ __forceinline__ T block_exclusive_scan(T v, T* wave_sums, T* total) {
  const int lane = lane_id(), w = (int)(threadIdx.x >> 6);
  T x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T y = __shfl_up(x, (unsigned)o, 64);
    if (lane >= o) x += y;
  }
  if (lane == 63) wave_sums[w] = x;
  __syncthreads();
  T base = 0, tot = 0;
#pragma unroll
  for (int k = 0; k < kScanWaves; ++k) {
    const T s = wave_sums[k];
    if (k < w) base += s;
    tot += s;
  }
  __syncthreads();   // wave_sums may be reused
  *total = tot;
  return base + x - v;
}

// One workgroup: exclusive scan of sums[0, n) in place, *total = the grand total (sums + n where it follows the totals).  A round
// takes one total per thread and carries the running total into the next.
template <typename T>
__device__ __forceinline__ void scan_totals_in_place(T* sums, int64_t n, T* total, T* lds) {
  T carry = 0, tot;
  for (int64_t c0 = 0; c0 < n; c0 += kScanBlock) {
    const int64_t t = c0 + threadIdx.x;
    const T v = t < n ? sums[t] : 0;
    const T pre = block_exclusive_scan<T>(v, lds, &tot) + carry;
    if (t < n) sums[t] = pre;
    carry += tot;
  }
  if (threadIdx.x == 0) *total = carry;
}

// One workgroup: exclusive scan of row[0, ntiles) in place (the per-tile counts of one digit or partition), offset by
// `before`, the items of the smaller ids.  A round takes ITEMS counts per thread.
template <int ITEMS>
__device__ __forceinline__ void scan_count_rows(uint32_t* row, int64_t ntiles, uint32_t before, uint32_t* lds) {
  uint32_t carry = before, tot;
  for (int64_t c0 = 0; c0 < ntiles; c0 += kScanBlock * ITEMS) {
    const int64_t at = c0 + (int64_t)threadIdx.x * ITEMS;
    uint32_t v[ITEMS], s = 0;
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) { v[k] = at + k < ntiles ? row[at + k] : 0; s += v[k]; }
    uint32_t pre = block_exclusive_scan<uint32_t>(s, lds, &tot) + carry;
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
      if (at + k < ntiles) row[at + k] = pre;
      pre += v[k];
    }
    carry += tot;
  }
}

// Arrow bitmap words (LSB first) of one predicate per row: words[w] = the ballot of pred(64 w + lane) over the rows below n.
// A wave per word, grid-stride.
template <class Pred>
__device__ __forceinline__ void pack_ballot_words(void* words, int64_t n, Pred pred) {
  const int64_t nwords = (n + 63) >> 6;
  for (int64_t w = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; w < nwords; w += ((int64_t)gridDim.x * blockDim.x) >> 6) {
    const int64_t r = (w << 6) + lane_id();
    const uint64_t m = __ballot(r < n && pred(r));
    if (lane_id() == 0) ((uint64_t*)words)[w] = m;
  }
}

// Eight lanes (sl = 0 .. 7) copy the len bytes of one row: 16-byte chunks, then the tail byte by byte.  (Source and destination
// are only byte aligned: the chunks go through memcpy, global memory takes unaligned accesses.)
__device__ __forceinline__ void copy_row_by_8_lanes(uint8_t* dst, const uint8_t* src, uint32_t len, int sl) {
  for (uint32_t b = (uint32_t)sl * 16; b + 16 <= len; b += 128) { uint4 w; __builtin_memcpy(&w, src + b, 16); __builtin_memcpy(dst + b, &w, 16); }
  for (uint32_t k = (len & ~15u) + sl; k < len; k += 8) dst[k] = src[k];
}

// lanes of this wave whose `d` (8 bits) equals this lane's, among the lanes in `active`
__device__ __forceinline__ uint64_t byte_peers(uint32_t d, uint64_t active) {
  uint64_t peers = active;
#pragma unroll
  for (int b = 0; b < 8; ++b) {
    const uint64_t m = __ballot((d >> b) & 1);
    peers &= ((d >> b) & 1) ? m : ~m;
  }
  return peers;
}

// Where every item of a tile goes when the tile is ordered by an 8-bit id, stably.  Wave w owns the w-th quarter of the tile,
// item j of lane l being item wbase + j * 64 + l (wbase: the quarter's first item; items >= n do not exist); id_of(j) is this
// lane's id of item j.  wcnt must be zero and visible on entry.  On return pos[j] is the item's place in the tile, dstart[d]
// the place of id d's first item, and every thread has passed a barrier behind the last write of either.
template <int ITEMS, class IdOf>
__device__ __forceinline__ void tile_positions(IdOf id_of, int64_t wbase, int64_t n, uint32_t (*wcnt)[256], uint32_t* dstart,
                                               uint32_t* lds, uint32_t (&pos)[ITEMS]) {
  const int w = (int)(threadIdx.x >> 6);
#pragma unroll
  for (int j = 0; j < ITEMS; ++j) {
    const bool valid = wbase + j * 64 + lane_id() < n;
    const uint32_t d = id_of(j);
    const uint64_t peers = byte_peers(d, __ballot(valid));
    const uint32_t before = wcnt[w][d];
    pos[j] = before + (uint32_t)__popcll(peers & lanes_below());
    // one lane per id moves the wave's counter on; every lane of the wave has read it above (LDS is in order per wave)
    if (valid && (peers & lanes_below()) == 0) wcnt[w][d] = before + (uint32_t)__popcll(peers);
  }
  __syncthreads();
  {   // per id: offsets of the waves inside the id's run, and where the run starts in the tile
    const int d = threadIdx.x;
    uint32_t s = 0;
#pragma unroll
    for (int k = 0; k < kScanWaves; ++k) { const uint32_t c = wcnt[k][d]; wcnt[k][d] = s; s += c; }
    uint32_t total;
    dstart[d] = block_exclusive_scan<uint32_t>(s, lds, &total);
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < ITEMS; ++j) {
    const uint32_t d = id_of(j);
    pos[j] += dstart[d] + wcnt[w][d];
  }
}

}  // namespace chq
