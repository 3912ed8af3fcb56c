// temporal.hip -- gfx950 kernels of EXTRACT / date_part and date_trunc.  Like the other typed operations
// they write a temporary column that replaces the node before the rest of the expression is lowered.
//
//   temporal_part_kernel<KIND>    Int32 / Int64 raw values -> an Int32 column holding one calendar or clock field
//   temporal_trunc_kernel<KIND>   Int32 / Int64 raw values -> a column of the same width, truncated to a unit
// One instantiation per source kind, chosen once per launch: the units per day, hour, minute and second are compile-time
// constants of it, so no division instruction sequence is generated (temporal_device.h).  The field / unit is wave-uniform.  Both
// are on the row loop and the validity epilogue of wave_rows.h: a wave owns 64 consecutive rows, lane 0 stores their validity
// word from one ballot and adds the wave's nulls with at most one atomic; a null row is written as 0.  The grid is capped at
// TEMPORAL_GRID_CAP.  Every load is the value of a row i < nrows at element values_offset + i (the value of a null row is read --
// it lies inside the buffer -- but never judged).
#include <hip/hip_runtime.h>

#include "temporal_device.h"
#include "typed_ops.h"   // rows_grid
#include "wave_rows.h"

namespace chq {
namespace {
typedef unsigned long long u64;

template <int KIND>
__device__ __forceinline__ int64_t load_raw(const void* values, int64_t at) {
  return temporal_is_i32(KIND) ? (int64_t)((const int32_t*)values)[at] : ((const int64_t*)values)[at];
}

template <int KIND>
__global__ __launch_bounds__(kRowsBlock) void temporal_part_kernel(const TemporalParams p) {
  const int64_t nrows = p.nrows;
  const int field = p.op;
  int32_t* const out_values = (int32_t*)p.out_values;
  CHQ_FOR_WAVE_ROWS(base, nrows) {
    const int64_t i = base + lane_id();
    bool valid = false;
    int32_t out = 0;
    if (i < nrows) valid = row_valid(p.validity, p.validity_offset, i) && temporal_part_of<KIND>(field, load_raw<KIND>(p.values, p.values_offset + i), &out);
    if (i < nrows) out_values[i] = valid ? out : 0;
    store_validity_word(p.out_validity, p.null_count, base, wave_rows_end(nrows, base), __ballot(valid));
  }
}

template <int KIND>
__global__ __launch_bounds__(kRowsBlock) void temporal_trunc_kernel(const TemporalParams p) {
  const int64_t nrows = p.nrows;
  const int unit = p.op;
  CHQ_FOR_WAVE_ROWS(base, nrows) {
    const int64_t i = base + lane_id();
    bool valid = false;
    int64_t out = 0;
    if (i < nrows) valid = row_valid(p.validity, p.validity_offset, i) && temporal_trunc_of<KIND>(unit, load_raw<KIND>(p.values, p.values_offset + i), &out);
    if (i < nrows) {
      if (temporal_is_i32(KIND)) ((int32_t*)p.out_values)[i] = valid ? (int32_t)out : 0;
      else ((int64_t*)p.out_values)[i] = valid ? out : 0;
    }
    store_validity_word(p.out_validity, p.null_count, base, wave_rows_end(nrows, base), __ballot(valid));
  }
}
}  // namespace

hipError_t launch_temporal_part(const TemporalParams& p, hipStream_t stream) {
  const dim3 grid(rows_grid(p.nrows, TEMPORAL_GRID_CAP)), block(kRowsBlock);
#define CHQ_TEMPORAL_CASE(K) \
  case K: hipLaunchKernelGGL((temporal_part_kernel<K>), grid, block, 0, stream, p); break;
  switch (p.kind == TK_DATE64 ? (int32_t)TK_TS_MS : p.kind) {   // (Date64 is read as milliseconds)
    CHQ_TEMPORAL_CASE(TK_DATE32) CHQ_TEMPORAL_CASE(TK_TS_S) CHQ_TEMPORAL_CASE(TK_TS_MS) CHQ_TEMPORAL_CASE(TK_TS_US) CHQ_TEMPORAL_CASE(TK_TS_NS)
    CHQ_TEMPORAL_CASE(TK_TIME32_S) CHQ_TEMPORAL_CASE(TK_TIME32_MS) CHQ_TEMPORAL_CASE(TK_TIME64_US) CHQ_TEMPORAL_CASE(TK_TIME64_NS)
    default: return hipErrorInvalidValue;
  }
#undef CHQ_TEMPORAL_CASE
  return hipGetLastError();
}
hipError_t launch_temporal_trunc(const TemporalParams& p, hipStream_t stream) {
  const dim3 grid(rows_grid(p.nrows, TEMPORAL_GRID_CAP)), block(kRowsBlock);
#define CHQ_TEMPORAL_CASE(K) \
  case K: hipLaunchKernelGGL((temporal_trunc_kernel<K>), grid, block, 0, stream, p); break;
  switch (p.kind == TK_DATE64 ? (int32_t)TK_TS_MS : p.kind) {
    CHQ_TEMPORAL_CASE(TK_DATE32) CHQ_TEMPORAL_CASE(TK_TS_S) CHQ_TEMPORAL_CASE(TK_TS_MS) CHQ_TEMPORAL_CASE(TK_TS_US) CHQ_TEMPORAL_CASE(TK_TS_NS)
    default: return hipErrorInvalidValue;
  }
#undef CHQ_TEMPORAL_CASE
  return hipGetLastError();
}
}  // namespace chq
