// cast.hip -- gfx950 kernels of CAST / TRY_CAST.  Like the other typed operations they write a
// temporary column that replaces the node before the rest of the expression is lowered.
//
//   cast_fixed_kernel<S, D>   Boolean / integer / float -> Boolean / integer / float, one instantiation per (source class,
//                             target class); the type inside the class (width, signedness) is a wave-uniform parameter.
//   cast_parse_kernel         Utf8 -> integer, a lane per row looping over the row's bytes (rows are short; a long row is
//                             leading zeros or a failure).
//   cast_len_kernel           integer / Boolean -> Utf8, step 1: the byte length of every row from the value alone.
//   (scan.hip)                step 2: launch_offsets_scan -> Int32 offsets and the 64-bit byte total.
//   cast_write_kernel         step 3: every lane writes its row's bytes at its offset.
// The first three are on the row loop of wave_rows.h but not on its epilogue: nothing here is written with atomics, null counts
// come from count_bits_kernel over the output validity, and lane 0 stores the validity word and the failure flag in one block (a
// failing VALID row of a CAST makes it store 1 into the flag word: a plain vector store, every writer writes the same value).
// The grid of all four is capped at CAST_GRID_CAP.
// Every load of string data is a byte load inside [offsets[i], offsets[i + 1]) of a VALID row i < nrows.
#include <hip/hip_runtime.h>

#include "cast_device.h"
#include "typed_ops.h"   // rows_grid
#include "wave_rows.h"

namespace chq {
namespace {
typedef unsigned long long u64;
static_assert(CAST_BLOCK == kRowsBlock, "cast.hip runs on the row loop and the grid of wave_rows.h");

enum CastClass { CC_BOOL = 0, CC_INT = 1, CC_FLOAT = 2 };

// the value of row i as 64 bits (cast_device.h): integers extended by their signedness, floats as their pattern
template <int S>
__device__ __forceinline__ uint64_t load_value(const void* values, int64_t values_offset, int64_t i, int from) {
  if (S == CC_BOOL) return bit_at(values, values_offset + i) ? 1 : 0;
  const uint8_t* v = (const uint8_t*)values;
  if (S == CC_INT && cast_is_signed(from)) {
    switch (cast_width(from)) {
      case 1: return (uint64_t)(int64_t)((const int8_t*)v)[i];
      case 2: return (uint64_t)(int64_t)((const int16_t*)v)[i];
      case 4: return (uint64_t)(int64_t)((const int32_t*)v)[i];
      default: return ((const uint64_t*)v)[i];
    }
  }
  switch (cast_width(from)) {
    case 1: return v[i];
    case 2: return ((const uint16_t*)v)[i];
    case 4: return ((const uint32_t*)v)[i];
    default: return ((const uint64_t*)v)[i];
  }
}
__device__ __forceinline__ void store_value(void* out, int64_t i, int width, uint64_t bits) {
  switch (width) {
    case 1: ((uint8_t*)out)[i] = (uint8_t)bits; break;
    case 2: ((uint16_t*)out)[i] = (uint16_t)bits; break;
    case 4: ((uint32_t*)out)[i] = (uint32_t)bits; break;
    default: ((uint64_t*)out)[i] = bits; break;
  }
}

template <int S, int D>
__global__ __launch_bounds__(CAST_BLOCK) void cast_fixed_kernel(const CastFixedParams p) {
  const int width = cast_width(p.to);
  CHQ_FOR_WAVE_ROWS(base, p.nrows) {
    const int64_t i = base + lane_id();
    bool valid = false, ok = false;
    uint64_t out = 0;
    if (i < p.nrows) {
      valid = row_valid(p.validity, p.validity_offset, i);
      // (the value of a null row is read -- it lies inside the buffer -- but never judged)
      ok = cast_fixed_value(load_value<S>(p.values, p.values_offset, i, p.from), p.from, p.to, &out);
    }
    const u64 vm = __ballot(valid && ok), fm = __ballot(valid && !ok);
    if (!(valid && ok)) out = 0;
    if (D == CC_BOOL) {
      const u64 rm = __ballot(out != 0);
      if (lane_id() == 0) ((u64*)p.out_values)[base >> 6] = rm;
    } else if (i < p.nrows) {
      store_value(p.out_values, i, width, out);
    }
    if (lane_id() == 0) {
      p.out_validity[base >> 6] = vm;
      if (fm != 0 && !p.try_cast) *p.fail = 1u;
    }
  }
}

__global__ __launch_bounds__(CAST_BLOCK) void cast_parse_kernel(const CastParseParams p) {
  const int width = cast_width(p.to);
  CHQ_FOR_WAVE_ROWS(base, p.nrows) {
    const int64_t i = base + lane_id();
    bool valid = false, ok = false;
    uint64_t out = 0;
    if (i < p.nrows && row_valid(p.validity, p.validity_offset, i)) {
      valid = true;
      const int32_t b = p.offsets[i], e = p.offsets[i + 1];
      ok = cast_parse_int(p.data + b, e - b, p.to, &out);
    }
    const u64 vm = __ballot(valid && ok), fm = __ballot(valid && !ok);
    if (i < p.nrows) store_value(p.out_values, i, width, ok ? out : 0);
    if (lane_id() == 0) {
      p.out_validity[base >> 6] = vm;
      if (fm != 0 && !p.try_cast) *p.fail = 1u;
    }
  }
}

template <int S>
__global__ __launch_bounds__(CAST_BLOCK) void cast_len_kernel(const CastPrintParams p) {
  CHQ_FOR_WAVE_ROWS(base, p.nrows) {
    const int64_t i = base + lane_id();
    bool valid = false;
    uint32_t len = 0;
    if (i < p.nrows && row_valid(p.validity, p.validity_offset, i)) {
      valid = true;
      const uint64_t v = load_value<S>(p.values, p.values_offset, i, p.from);
      len = (uint32_t)(S == CC_BOOL ? cast_bool_len(v != 0) : cast_decimal_len(v, cast_is_signed(p.from)));
    }
    const u64 vm = __ballot(valid);
    if (i < p.nrows) p.out_len[i] = len;
    if (lane_id() == 0) p.out_validity[base >> 6] = vm;
  }
}

template <int S>
__global__ __launch_bounds__(CAST_BLOCK) void cast_write_kernel(const CastPrintParams p) {
  for (int64_t i = (int64_t)blockIdx.x * CAST_BLOCK + threadIdx.x; i < p.nrows; i += (int64_t)gridDim.x * CAST_BLOCK) {
    const int32_t b = p.out_offsets[i], n = p.out_offsets[i + 1] - b;
    if (n <= 0) continue;   // a null row
    const uint64_t v = load_value<S>(p.values, p.values_offset, i, p.from);
    if (S == CC_BOOL) cast_write_bool(v != 0, p.out_data + b);
    else cast_write_decimal(v, cast_is_signed(p.from), p.out_data + b, n);
  }
}

int class_of(int t) { return t == CT_BOOL ? CC_BOOL : cast_is_int(t) ? CC_INT : CC_FLOAT; }
}  // namespace

hipError_t launch_cast_fixed(const CastFixedParams& p, hipStream_t stream) {
  const dim3 grid(rows_grid(p.nrows, CAST_GRID_CAP)), block(CAST_BLOCK);
#define CHQ_CAST_CASE(S, D) \
  case (S) * 3 + (D): hipLaunchKernelGGL((cast_fixed_kernel<S, D>), grid, block, 0, stream, p); break;
  switch (class_of(p.from) * 3 + class_of(p.to)) {
    CHQ_CAST_CASE(CC_BOOL, CC_BOOL) CHQ_CAST_CASE(CC_BOOL, CC_INT) CHQ_CAST_CASE(CC_BOOL, CC_FLOAT)
    CHQ_CAST_CASE(CC_INT, CC_BOOL) CHQ_CAST_CASE(CC_INT, CC_INT) CHQ_CAST_CASE(CC_INT, CC_FLOAT)
    CHQ_CAST_CASE(CC_FLOAT, CC_BOOL) CHQ_CAST_CASE(CC_FLOAT, CC_INT) CHQ_CAST_CASE(CC_FLOAT, CC_FLOAT)
    default: return hipErrorInvalidValue;
  }
#undef CHQ_CAST_CASE
  return hipGetLastError();
}
hipError_t launch_cast_parse(const CastParseParams& p, hipStream_t stream) {
  hipLaunchKernelGGL(cast_parse_kernel, dim3(rows_grid(p.nrows, CAST_GRID_CAP)), dim3(CAST_BLOCK), 0, stream, p);
  return hipGetLastError();
}
hipError_t launch_cast_len(const CastPrintParams& p, hipStream_t stream) {
  if (p.from == CT_BOOL) hipLaunchKernelGGL(cast_len_kernel<CC_BOOL>, dim3(rows_grid(p.nrows, CAST_GRID_CAP)), dim3(CAST_BLOCK), 0, stream, p);
  else hipLaunchKernelGGL(cast_len_kernel<CC_INT>, dim3(rows_grid(p.nrows, CAST_GRID_CAP)), dim3(CAST_BLOCK), 0, stream, p);
  return hipGetLastError();
}
hipError_t launch_cast_write(const CastPrintParams& p, hipStream_t stream) {
  if (p.from == CT_BOOL) hipLaunchKernelGGL(cast_write_kernel<CC_BOOL>, dim3(rows_grid(p.nrows, CAST_GRID_CAP)), dim3(CAST_BLOCK), 0, stream, p);
  else hipLaunchKernelGGL(cast_write_kernel<CC_INT>, dim3(rows_grid(p.nrows, CAST_GRID_CAP)), dim3(CAST_BLOCK), 0, stream, p);
  return hipGetLastError();
}
}  // namespace chq
