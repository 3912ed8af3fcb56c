// like.hip -- gfx950 kernel of `column [NOT] LIKE 'pattern'`: a temporary Boolean column on the
// row-wise scheme of wave_rows.h.  The matcher is like_device.h's, the same code the host folds literals with.
//
// Two modes, picked per wave from the bytes its rows span (wave_spans_more_than, no host decision):
//   lane per row   each lane runs like_match on its own row.  Patterns whose `%` stand only at the ends (`abc%`, `%abc`,
//                  none at all) are decided by like_ends alone, which reads the two ends and never the body.
//   wave per row   more than LIKE_WAVE_MODE_BYTES in the wave and the pattern has pieces to search for: the wave takes its
//                  rows one after the other; per step lane l tries the piece at position pos + l (neighbouring lanes read
//                  neighbouring bytes), and the LEFTMOST hit of the ballot moves pos behind the piece.
// Every load of string data is a byte load inside [offsets[i], offsets[i + 1]) of a VALID row i < nrows: no padding is
// assumed, and the offsets of null rows may enclose anything.
#include <hip/hip_runtime.h>

#include "like_device.h"
#include "typed_ops.h"   // rows_grid
#include "wave_rows.h"

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

__global__ __launch_bounds__(kRowsBlock) void like_kernel(const LikeParams p) {
  const int lane = lane_id();
  const bool has_middle = p.pat.first_end < p.pat.last_begin;
  CHQ_FOR_WAVE_ROWS(base, p.nrows) {
    const int64_t i = base + lane_id(), wave_end = wave_rows_end(p.nrows, base);
    bool valid = false, r = false;
    int32_t b = 0, e = 0;
    if (i < p.nrows) {
      valid = row_valid(p.validity, p.validity_offset, i);
      b = p.offsets[i]; e = p.offsets[i + 1];
    }
    const u64 vm = __ballot(valid);
    if (has_middle && wave_spans_more_than(p.offsets, base, wave_end, LIKE_WAVE_MODE_BYTES)) {
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
    if (lane == 0) p.out_bits[base >> 6] = rm;
    store_validity_word(p.out_validity, p.null_count, base, wave_end, vm);
  }
}
}  // namespace

hipError_t launch_like(const LikeParams& p, hipStream_t stream) {
  hipLaunchKernelGGL(like_kernel, dim3(rows_grid(p.nrows, 256 * 32)), dim3(256), 0, stream, p);
  return hipGetLastError();
}
}  // namespace chq
