// like.hip -- gfx950 kernel of `column [NOT] LIKE 'pattern'`.  Like the other typed operations
// (typed_ops.hip) it writes a temporary Boolean column: one wave owns 64 consecutive rows and stores one 64-bit value word
// and one validity word from ballots; the null count takes one atomic per wave.  The matcher is like_device.h's, the same
// code the host folds literals with.
//
// Two modes, picked per wave from the bytes its 64 rows span (offsets[base + 64] - offsets[base], no host decision):
//   lane per row   each lane runs like_match on its own row.  Patterns whose `%` stand only at the ends (`abc%`, `%abc`,
//                  none at all) are decided by like_ends alone, which reads the two ends and never the body.
//   wave per row   more than LIKE_WAVE_MODE_BYTES in the wave and the pattern has pieces to search for: the wave takes its
//                  rows one after the other; per step lane l tries the piece at position pos + l (neighbouring lanes read
//                  neighbouring bytes), and the LEFTMOST hit of the ballot moves pos behind the piece.
// Every load of string data is a byte load inside [offsets[i], offsets[i + 1]) of a VALID row i < nrows: no padding is
// assumed, and the offsets of null rows may enclose anything.
#include <hip/hip_runtime.h>

#include "like_device.h"
#include "scan_device.h"   // bit_at

namespace chq {
namespace {
typedef unsigned long long u64;

// the pieces between the anchored ones, found by the whole wave in s[pos, lim): every argument is wave-uniform
__device__ bool wave_search(const LikePattern& pat, const uint8_t* s, int32_t pos, int32_t lim, int lane) {
  for (int eb = pat.first_end; eb < pat.last_begin;) {
    const int ee = like_piece_end(pat, eb);
    int32_t next = -1;
    for (; pos + (ee - eb) <= lim; pos += 64) {
      const int32_t cand = pos + lane;
      const int32_t e = cand + (ee - eb) <= lim ? like_piece_at(pat, eb, ee, s, cand, lim) : -1;
      const u64 hits = __ballot(e >= 0);
      if (hits) { next = __shfl(e, __ffsll((long long)hits) - 1); break; }   // the leftmost candidate, never "any"
    }
    if (next < 0) return false;
    pos = next;
    eb = ee;
  }
  return true;
}

__global__ __launch_bounds__(256) void like_kernel(const LikeParams p) {
  const int lane = threadIdx.x & 63;
  const bool has_middle = p.pat.first_end < p.pat.last_begin;
  for (int64_t base = ((int64_t)blockIdx.x * 256 + threadIdx.x) & ~63LL; base < p.nrows; base += (int64_t)gridDim.x * 256) {
    const int64_t i = base + lane;
    const int64_t wave_end = p.nrows - base < 64 ? p.nrows : base + 64;   // (no offset of a row >= nrows is read)
    bool valid = false, r = false;
    int32_t b = 0, e = 0;
    if (i < p.nrows) {
      valid = !p.validity || bit_at(p.validity, p.validity_offset + i);
      b = p.offsets[i]; e = p.offsets[i + 1];
    }
    const u64 vm = __ballot(valid);
    if (has_middle && (int64_t)p.offsets[wave_end] - (int64_t)p.offsets[base] > LIKE_WAVE_MODE_BYTES) {
      for (u64 todo = vm; todo; todo &= todo - 1) {
        const int row = __ffsll((long long)todo) - 1;
        const int32_t rb = __shfl(b, row), re = __shfl(e, row);
        int32_t pos, lim;
        bool m = like_ends(p.pat, p.data + rb, re - rb, &pos, &lim);
        if (m) m = wave_search(p.pat, p.data + rb, pos, lim, lane);
        if (lane == row) r = m;
      }
    } else if (valid) {
      r = like_match(p.pat, p.data + b, e - b);
    }
    const u64 rm = __ballot(valid && (r != (p.negated != 0)));
    if (lane == 0) {
      p.out_bits[base >> 6] = rm;
      p.out_validity[base >> 6] = vm;
      const unsigned nulls = (unsigned)(wave_end - base) - (unsigned)__popcll(vm);
      if (nulls) atomicAdd(p.null_count, (u64)nulls);
    }
  }
}
}  // namespace

hipError_t launch_like(const LikeParams& p, hipStream_t stream) {
  const int64_t blocks = (p.nrows + 255) / 256;
  hipLaunchKernelGGL(like_kernel, dim3((unsigned)(blocks < 1 ? 1 : blocks > 256 * 32 ? 256 * 32 : blocks)), dim3(256), 0, stream, p);
  return hipGetLastError();
}
}  // namespace chq
