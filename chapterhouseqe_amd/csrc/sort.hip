// sort.hip -- the ORDER BY kernels (gfx950, wave64): key-word normalisation, the LSD radix passes over (u64 key, u32 row)
// pairs and the gathers that apply the final permutation to every column.  Host side: sort.cpp.
//
// A radix pass is three launches that hand data over only at launch boundaries (count -> scan -> scatter): no workgroup
// waits on another inside a launch, so nothing spins and nothing depends on dispatch order.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "scan_device.h"
#include "sort_device.h"

namespace chq {
namespace {

constexpr int kWaves = kScanWaves;
static_assert(kSortBlock == kScanBlock && kSortItems == kScanItems && kSortTile == kScanTile, "the sort's tiles are the shared scan geometry");

// ---- key words ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kSortBlock) void sort_norm_kernel(const SortNormParams p) {
  const int64_t i = (int64_t)blockIdx.x * kSortBlock + threadIdx.x;
  if (i >= p.n) return;
  const uint32_t r = p.perm ? p.perm[i] : (uint32_t)i;
  const bool valid = !p.validity || bit_at(p.validity, p.bit_offset + r);
  uint64_t k = 0;
  if (p.kind == SW_NULL_FLAG) {
    k = valid == (p.nulls_first != 0) ? 1 : 0;
  } else if (valid) {
    switch (p.kind) {
      case SW_SIGNED: k = (uint64_t)load_int(p.values, r, p.width) ^ (1ull << 63); break;
      case SW_UNSIGNED: k = load_uint(p.values, r, p.width); break;
      case SW_FLOAT: {
        const int bits = 8 * p.width;
        const uint64_t u = load_uint(p.values, r, p.width);
        const uint64_t sign = 1ull << (bits - 1), mask = bits == 64 ? ~0ull : (1ull << bits) - 1;
        k = (u & sign) ? (~u & mask) : (u | sign);
        break;
      }
      case SW_BOOL: k = bit_at(p.values, p.bit_offset + r) ? 1 : 0; break;
      case SW_DEC_LO: k = ((const uint64_t*)p.values)[2 * (uint64_t)r]; break;
      case SW_DEC_HI: k = ((const uint64_t*)p.values)[2 * (uint64_t)r + 1] ^ (1ull << 63); break;
      case SW_UTF8_LEN: {
        const int32_t* offs = (const int32_t*)p.values;
        k = (uint64_t)(uint32_t)(offs[r + 1] - offs[r]);
        break;
      }
      case SW_UTF8_CHUNK: {
        const int32_t* offs = (const int32_t*)p.values;
        const int64_t len = offs[r + 1] - offs[r], at = 8 * p.chunk;
        const uint8_t* s = p.data + offs[r] + at;
        const int64_t take = len - at < 0 ? 0 : (len - at > 8 ? 8 : len - at);
        for (int64_t b = 0; b < take; ++b) k |= (uint64_t)s[b] << (56 - 8 * b);
        break;
      }
      default: break;
    }
    k ^= p.invert;
  }
  p.keys[i] = k;
  p.vals[i] = r;
}

// every byte's histogram in one read of the keys; a wave whose lanes agree on a byte adds once (constant bytes are common)
__global__ __launch_bounds__(kSortBlock) void sort_hist_kernel(const SortHistParams p) {
  __shared__ uint32_t h[8][256];
  for (int k = threadIdx.x; k < 8 * 256; k += kSortBlock) (&h[0][0])[k] = 0;
  __syncthreads();
  const int64_t stride = (int64_t)gridDim.x * kSortBlock;
  const int64_t first = (int64_t)blockIdx.x * kSortBlock + (threadIdx.x & ~63);   // wave-uniform
  for (int64_t base = first; base < p.n; base += stride) {
    const int64_t i = base + lane_id();
    const bool valid = i < p.n;
    const uint64_t key = valid ? p.keys[i] : 0;
    const uint64_t active = __ballot(valid);
    const uint32_t cnt = (uint32_t)__popcll(active);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const uint32_t d = (uint32_t)(key >> (8 * b)) & 255;
      const uint32_t d0 = __shfl(d, 0, 64);   // lane 0 is active whenever any lane is
      if (__all(!valid || d == d0)) {
        if (lane_id() == 0) atomicAdd(&h[b][d0], cnt);
      } else if (valid) {
        atomicAdd(&h[b][d], 1u);
      }
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < 8 * 256; k += kSortBlock) {
    const uint32_t c = (&h[0][0])[k];
    if (c) atomicAdd(&p.hist[k], c);
  }
}

// ---- one radix pass: count -> scan -> scatter ----------------------------------------------------------------------------
// Tile t = pairs [t kSortTile, (t+1) kSortTile); wave w of its workgroup owns the w-th quarter, item j of lane l being pair
// w * kSortTile/4 + j * 64 + l.  Both the count and the scatter rank items in that order, which is the input order: stable.
__global__ __launch_bounds__(kSortBlock) void sort_count_kernel(const SortPassParams p) {
  __shared__ uint32_t cnt[256];
  cnt[threadIdx.x] = 0;
  __syncthreads();
  const int64_t tile = blockIdx.x;
  const int64_t wbase = tile * kSortTile + (int64_t)(threadIdx.x >> 6) * (kSortTile / kWaves);
#pragma unroll
  for (int j = 0; j < kSortItems; ++j) {
    const int64_t i = wbase + j * 64 + lane_id();
    const bool valid = i < p.n;
    const uint32_t d = valid ? (uint32_t)(p.keys_in[i] >> p.shift) & 255 : 0;
    const uint64_t peers = byte_peers(d, __ballot(valid));
    if (valid && (peers & lanes_below()) == 0) atomicAdd(&cnt[d], (uint32_t)__popcll(peers));
  }
  __syncthreads();
  p.tile_counts[(int64_t)threadIdx.x * p.ntiles + tile] = cnt[threadIdx.x];
}

// workgroup d: exclusive scan of digit d's tile counts, offset by the keys of the smaller digits
__global__ __launch_bounds__(kSortBlock) void sort_scan_kernel(const SortPassParams p) {
  __shared__ uint32_t sums[kWaves];
  const int d = blockIdx.x;
  const uint32_t before = block_sum<uint32_t>(threadIdx.x < (unsigned)d ? p.digit_hist[threadIdx.x] : 0u, sums);
  scan_count_rows<kSortItems>(p.tile_counts + (int64_t)d * p.ntiles, p.ntiles, before, sums);
}

// ranks every pair of the tile, stages the tile in LDS in digit order, then writes each digit's run contiguously
__global__ __launch_bounds__(kSortBlock) void sort_scatter_kernel(const SortPassParams p) {
  __shared__ uint64_t sk[kSortTile];
  __shared__ uint32_t sv[kSortTile];
  __shared__ uint32_t wcnt[kWaves][256];
  __shared__ uint32_t dstart[256];
  __shared__ uint32_t gbase[256];
  __shared__ uint32_t sums[kWaves];
  const int w = (int)(threadIdx.x >> 6);
  for (int k = threadIdx.x; k < kWaves * 256; k += kSortBlock) (&wcnt[0][0])[k] = 0;
  const int64_t tile = blockIdx.x;
  const int64_t tbase = tile * kSortTile;
  const int64_t wbase = tbase + (int64_t)w * (kSortTile / kWaves);
  uint64_t key[kSortItems];
  uint32_t val[kSortItems];
#pragma unroll
  for (int j = 0; j < kSortItems; ++j) {
    const int64_t i = wbase + j * 64 + lane_id();
    key[j] = i < p.n ? p.keys_in[i] : 0;
    val[j] = i < p.n ? p.vals_in[i] : 0;
  }
  __syncthreads();
  uint32_t pos[kSortItems];
  const uint32_t out0 = p.tile_counts[(int64_t)threadIdx.x * p.ntiles + tile];
  tile_positions<kSortItems>([&](int j) { return (uint32_t)(key[j] >> p.shift) & 255; }, wbase, p.n, wcnt, dstart, sums, pos);
  gbase[threadIdx.x] = out0 - dstart[threadIdx.x];   // (mod 2^32: gbase + position < 2^32)
#pragma unroll
  for (int j = 0; j < kSortItems; ++j) {
    if (wbase + j * 64 + lane_id() < p.n && pos[j] < (uint32_t)kSortTile) {
      sk[pos[j]] = key[j];
      sv[pos[j]] = val[j];
    }
  }
  __syncthreads();
  const int64_t left = p.n - tbase;
  const int tile_n = left < kSortTile ? (int)left : kSortTile;
  for (int q = threadIdx.x; q < tile_n; q += kSortBlock) {
    const uint64_t k = sk[q];
    const uint32_t dst = gbase[(uint32_t)(k >> p.shift) & 255] + (uint32_t)q;
    if ((int64_t)dst >= p.n) continue;   // (never taken: the positions of a pass are a permutation of [0, n))
    if (p.keys_out) p.keys_out[dst] = k;
    p.vals_out[dst] = sv[q];
  }
}

__global__ __launch_bounds__(kSortBlock) void sort_utf8_maxlen_kernel(const SortMaxLenParams p) {
  uint32_t mx = 0;
  for (int64_t i = (int64_t)blockIdx.x * kSortBlock + threadIdx.x; i < p.n; i += (int64_t)gridDim.x * kSortBlock) {
    const uint32_t len = (uint32_t)(p.offsets[i + 1] - p.offsets[i]);
    mx = len > mx ? len : mx;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const uint32_t y = __shfl_xor(mx, o, 64); mx = y > mx ? y : mx; }
  if (lane_id() == 0 && mx) atomicMax(p.out, mx);
}

// ---- gathers ---------------------------------------------------------------------------------------------------------------
// Every gather kernel that reads the row-id list exists in two compile-time variants.  kPad = false: the list holds rows only
// (ORDER BY, GROUP BY, partitioning, INNER JOIN).  kPad = true: the list may hold kSortNoRow, "no row" (the padded side of an
// outer join): such an output row is null -- validity bit 0, zero value bytes, Boolean bit 0, Utf8 length 0 -- and nothing of
// the source is read for it.
__device__ __forceinline__ uint32_t src_row(const SortGatherParams& p, int64_t i) { return p.perm ? p.perm[i] : (uint32_t)i; }

template <int W>
struct Word { uint8_t b[W]; };
template <>
struct Word<16> { uint64_t lo, hi; };

template <int W, bool kPad>
__global__ __launch_bounds__(kSortBlock) void sort_gather_fixed_kernel(const SortGatherParams p) {
  using T = typename std::conditional<W == 1, uint8_t, typename std::conditional<W == 2, uint16_t,
            typename std::conditional<W == 4, uint32_t, typename std::conditional<W == 8, uint64_t, Word<16>>::type>::type>::type>::type;
  const int64_t i = (int64_t)blockIdx.x * kSortBlock + threadIdx.x;
  if (i >= p.m) return;
  if constexpr (kPad) {
    const uint32_t r = src_row(p, i);
    T v{};
    if (r != kSortNoRow) v = ((const T*)p.in)[r];
    ((T*)p.out)[i] = v;
  } else {
    ((T*)p.out)[i] = ((const T*)p.in)[src_row(p, i)];
  }
}

// one output word of 32 bits per thread; set bits counted (null count of a validity bitmap).  kPad: a missing source bitmap
// (p.in null) is all ones, and "no row" gives a 0 bit.
template <bool kPad>
__global__ __launch_bounds__(kSortBlock) void sort_gather_bits_kernel(const SortGatherParams p) {
  const int64_t wi = (int64_t)blockIdx.x * kSortBlock + threadIdx.x;
  uint32_t word = 0;
  if (wi * 32 < p.m) {
    const int64_t i0 = wi * 32;
    const int n = p.m - i0 < 32 ? (int)(p.m - i0) : 32;
    if constexpr (kPad) {
      for (int b = 0; b < n; ++b) {
        const uint32_t r = src_row(p, i0 + b);
        word |= (uint32_t)(r != kSortNoRow && (!p.in || bit_at(p.in, p.in_bit_offset + r))) << b;
      }
    } else {
      for (int b = 0; b < n; ++b) word |= (uint32_t)bit_at(p.in, p.in_bit_offset + src_row(p, i0 + b)) << b;
    }
    ((uint32_t*)p.out)[wi] = word;
  }
  uint64_t ones = (uint64_t)__popc(word);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ones += __shfl_xor(ones, o, 64);
  if (p.ones && lane_id() == 0 && ones) atomicAdd((unsigned long long*)p.ones, (unsigned long long)ones);
}

template <bool kPad>
__device__ __forceinline__ uint64_t gathered_len(const SortGatherParams& p, int64_t i) {
  if (i >= p.m) return 0;
  const int32_t* offs = (const int32_t*)p.in;
  const uint32_t r = src_row(p, i);
  if constexpr (kPad) {
    if (r == kSortNoRow) return 0;
  }
  return (uint64_t)(uint32_t)(offs[r + 1] - offs[r]);
}

// Utf8 step 1: bytes of every output tile
template <bool kPad>
__global__ __launch_bounds__(kSortBlock) void sort_utf8_tile_sums_kernel(const SortGatherParams p) {
  __shared__ uint64_t sums[kWaves];
  const int64_t at = (int64_t)blockIdx.x * kSortTile + (int64_t)threadIdx.x * kSortItems;
  uint64_t s = 0;
#pragma unroll
  for (int k = 0; k < kSortItems; ++k) s += gathered_len<kPad>(p, at + k);
  const uint64_t tot = block_sum<uint64_t>(s, sums);
  if (threadIdx.x == 0) p.tile_sums[blockIdx.x] = tot;
}

// Utf8 step 2 (one workgroup): exclusive scan of the tile totals in place, the grand total behind them
__global__ __launch_bounds__(kSortBlock) void sort_utf8_scan_sums_kernel(const SortGatherParams p) {
  __shared__ uint64_t sums[kWaves];
  scan_totals_in_place<uint64_t>(p.tile_sums, p.ntiles, p.tile_sums + p.ntiles, sums);
}

// Utf8 step 3: output offsets (the host has checked that the grand total fits int32)
template <bool kPad>
__global__ __launch_bounds__(kSortBlock) void sort_utf8_offsets_kernel(const SortGatherParams p) {
  __shared__ uint64_t sums[kWaves];
  const int64_t at = (int64_t)blockIdx.x * kSortTile + (int64_t)threadIdx.x * kSortItems;
  uint64_t len[kSortItems], s = 0;
#pragma unroll
  for (int k = 0; k < kSortItems; ++k) { len[k] = gathered_len<kPad>(p, at + k); s += len[k]; }
  uint64_t tot;
  uint64_t pre = block_exclusive_scan<uint64_t>(s, sums, &tot) + p.tile_sums[blockIdx.x];
  int32_t* out = (int32_t*)p.out;
#pragma unroll
  for (int k = 0; k < kSortItems; ++k) {
    if (at + k < p.m) out[at + k] = (int32_t)pre;
    pre += len[k];
  }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) out[p.m] = (int32_t)p.tile_sums[p.ntiles];
}

// Utf8 step 4: bytes.  A lane copies a short string alone; the wave copies each long one together, 64 bytes a step.
// kPad: "no row" is a string of length 0 and copies nothing.
template <bool kPad>
__global__ __launch_bounds__(kSortBlock) void sort_utf8_copy_kernel(const SortGatherParams p) {
  constexpr int kShort = 32;
  const int64_t i = (int64_t)blockIdx.x * kSortBlock + threadIdx.x;
  const bool valid = i < p.m;
  const int32_t* in_offs = (const int32_t*)p.in;
  const int32_t* out_offs = (const int32_t*)p.out;
  int64_t src = 0, dst = 0, len = 0;
  if (valid) {
    const uint32_t r = src_row(p, i);
    if constexpr (kPad) {
      if (r != kSortNoRow) {
        src = in_offs[r];
        len = in_offs[r + 1] - src;
        dst = out_offs[i];
      }
    } else {
      src = in_offs[r];
      len = in_offs[r + 1] - src;
      dst = out_offs[i];
    }
  }
  if (valid && len <= kShort)
    for (int64_t b = 0; b < len; ++b) p.out_data[dst + b] = p.in_data[src + b];
  uint64_t longs = __ballot(valid && len > kShort);
  while (longs) {
    const int l = __ffsll((unsigned long long)longs) - 1;
    longs &= longs - 1;
    const int64_t s = __shfl(src, l, 64), t = __shfl(dst, l, 64), n = __shfl(len, l, 64);
    for (int64_t b = lane_id(); b < n; b += 64) p.out_data[t + b] = p.in_data[s + b];
  }
}

unsigned blocks_for(int64_t n, int64_t per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

hipError_t launch_sort_norm(const SortNormParams& p, hipStream_t stream) {
  hipLaunchKernelGGL(sort_norm_kernel, dim3(blocks_for(p.n, kSortBlock)), dim3(kSortBlock), 0, stream, p);
  return hipGetLastError();
}
hipError_t launch_sort_hist(const SortHistParams& p, int grid, hipStream_t stream) {
  const unsigned g = blocks_for(p.n, kSortBlock);
  hipLaunchKernelGGL(sort_hist_kernel, dim3(g < (unsigned)grid ? g : (unsigned)grid), dim3(kSortBlock), 0, stream, p);
  return hipGetLastError();
}
hipError_t launch_sort_pass(const SortPassParams& p, hipStream_t stream) {
  hipLaunchKernelGGL(sort_count_kernel, dim3((unsigned)p.ntiles), dim3(kSortBlock), 0, stream, p);
  hipLaunchKernelGGL(sort_scan_kernel, dim3(256), dim3(kSortBlock), 0, stream, p);
  hipLaunchKernelGGL(sort_scatter_kernel, dim3((unsigned)p.ntiles), dim3(kSortBlock), 0, stream, p);
  return hipGetLastError();
}
hipError_t launch_sort_utf8_maxlen(const SortMaxLenParams& p, int grid, hipStream_t stream) {
  const unsigned g = blocks_for(p.n, kSortBlock);
  hipLaunchKernelGGL(sort_utf8_maxlen_kernel, dim3(g < (unsigned)grid ? g : (unsigned)grid), dim3(kSortBlock), 0, stream, p);
  return hipGetLastError();
}
template <bool kPad>
void gather_fixed(const SortGatherParams& p, hipStream_t stream) {
  const dim3 g(blocks_for(p.m, kSortBlock)), b(kSortBlock);
  switch (p.width) {
    case 1: hipLaunchKernelGGL((sort_gather_fixed_kernel<1, kPad>), g, b, 0, stream, p); break;
    case 2: hipLaunchKernelGGL((sort_gather_fixed_kernel<2, kPad>), g, b, 0, stream, p); break;
    case 4: hipLaunchKernelGGL((sort_gather_fixed_kernel<4, kPad>), g, b, 0, stream, p); break;
    case 8: hipLaunchKernelGGL((sort_gather_fixed_kernel<8, kPad>), g, b, 0, stream, p); break;
    default: hipLaunchKernelGGL((sort_gather_fixed_kernel<16, kPad>), g, b, 0, stream, p); break;
  }
}
hipError_t launch_sort_gather_fixed(const SortGatherParams& p, hipStream_t stream, bool pad) {
  if (p.width != 1 && p.width != 2 && p.width != 4 && p.width != 8 && p.width != 16) return hipErrorInvalidValue;
  if (pad) gather_fixed<true>(p, stream);
  else gather_fixed<false>(p, stream);
  return hipGetLastError();
}
hipError_t launch_sort_gather_bits(const SortGatherParams& p, hipStream_t stream, bool pad) {
  const dim3 g(blocks_for(blocks_for(p.m, 32), kSortBlock)), b(kSortBlock);
  if (pad) hipLaunchKernelGGL(sort_gather_bits_kernel<true>, g, b, 0, stream, p);
  else hipLaunchKernelGGL(sort_gather_bits_kernel<false>, g, b, 0, stream, p);
  return hipGetLastError();
}
hipError_t launch_sort_utf8_sizes(const SortGatherParams& p, hipStream_t stream, bool pad) {   // steps 1 and 2
  if (pad) hipLaunchKernelGGL(sort_utf8_tile_sums_kernel<true>, dim3((unsigned)p.ntiles), dim3(kSortBlock), 0, stream, p);
  else hipLaunchKernelGGL(sort_utf8_tile_sums_kernel<false>, dim3((unsigned)p.ntiles), dim3(kSortBlock), 0, stream, p);
  hipLaunchKernelGGL(sort_utf8_scan_sums_kernel, dim3(1), dim3(kSortBlock), 0, stream, p);
  return hipGetLastError();
}
hipError_t launch_sort_utf8_copy(const SortGatherParams& p, hipStream_t stream, bool pad) {    // steps 3 and 4
  const dim3 g(blocks_for(p.m, kSortBlock)), b(kSortBlock);
  if (pad) {
    hipLaunchKernelGGL(sort_utf8_offsets_kernel<true>, dim3((unsigned)p.ntiles), b, 0, stream, p);
    hipLaunchKernelGGL(sort_utf8_copy_kernel<true>, g, b, 0, stream, p);
  } else {
    hipLaunchKernelGGL(sort_utf8_offsets_kernel<false>, dim3((unsigned)p.ntiles), b, 0, stream, p);
    hipLaunchKernelGGL(sort_utf8_copy_kernel<false>, g, b, 0, stream, p);
  }
  return hipGetLastError();
}

}  // namespace chq
