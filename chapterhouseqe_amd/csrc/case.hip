// case.hip -- gfx950 kernels of CASE / COALESCE / NULLIF.  Like the other typed operations they write
// a temporary column that replaces the node before the rest of the expression is lowered.  The rules are case_device.h's.
//
//   case_masks_kernel         one lane per 64 rows: the take mask of every WHEN and the remaining mask, aligned to bit 0
//   case_and_kernel           one lane per 64 rows: a bitmap re-aligned to bit 0 and ANDed with a guard (guarded views)
//   case_select_bool_kernel   one lane per 64 rows: a Boolean result from the masks and the branches' bitmaps
//   case_select_fixed_kernel  one lane per row, widths 1 / 2 / 4 / 8 / 16: the value of the chosen branch only
//   case_rows_kernel          one lane per row: byte length and validity of a Utf8 result (scan.hip turns them into offsets)
//   case_gather_kernel        the bytes of every Utf8 result row from its chosen source; lane per row, or wave per row when
//                             the wave's 64 rows hold more than CASE_WAVE_MODE_BYTES
// The last three are on the row-wise scheme of wave_rows.h; the first three launch on its grid, a lane per word.  Every launch
// is rows_grid(items, 256 * 32): one thread per item, `blocks > 256 * 32 ? 256 * 32 : blocks` workgroups (tests/test_gpu_case.py
// sizes its second-pass case from this line).
// Every load of a branch is of a row < nrows on which that branch is chosen and valid; every mask word index is below `words`.
#include <hip/hip_runtime.h>

#include "case_device.h"
#include "typed_ops.h"   // rows_grid
#include "wave_rows.h"

namespace chq {
namespace {
typedef unsigned long long u64;

__global__ __launch_bounds__(256) void case_masks_kernel(const CaseMasksParams p) {
  for (int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x; w < p.words; w += (int64_t)gridDim.x * 256) {
    u64* rem_word = p.masks + (int64_t)p.n_total * p.words + w;
    uint64_t remaining = p.first > 0 ? (uint64_t)*rem_word : case_rows_mask(w, p.nrows);
    for (int j = 0; j < p.n; ++j) {
      const CaseCond& c = p.cond[j];
      uint64_t cond = 0, valid = 0;
      if (c.kind == CASE_CONST) { valid = ~0ull; cond = c.const_val ? ~0ull : 0ull; }
      else if (c.kind == CASE_COLUMN && remaining) {
        valid = case_load_word(c.validity, c.offset, w, p.nrows);
        cond = case_load_word(c.values, c.offset, w, p.nrows);
      }
      p.masks[(int64_t)(p.first + j) * p.words + w] = case_take(&remaining, cond, valid);
    }
    *rem_word = remaining;
  }
}

__global__ __launch_bounds__(256) void case_and_kernel(const CaseAndParams p) {
  const int64_t words = (p.nrows + 63) >> 6;
  for (int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x; w < words; w += (int64_t)gridDim.x * 256) {
    const uint64_t g = p.guard ? (uint64_t)p.guard[w] : ~0ull;
    p.out[w] = g ? (case_load_word(p.bits, p.bit_off, w, p.nrows) & g) : 0ull;
  }
}

__global__ __launch_bounds__(256) void case_select_bool_kernel(const CaseSelectParams p) {
  unsigned nulls = 0;
  for (int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x; w < p.words; w += (int64_t)gridDim.x * 256) {
    uint64_t val, valid;
    case_select_bool_word(p, w, &val, &valid);
    ((u64*)p.out_values)[w] = val;
    p.out_validity[w] = valid;
    nulls += (unsigned)__popcll(case_rows_mask(w, p.nrows) & ~valid);
  }
  add_nulls(p.null_count, nulls);
}

template <int W>
__global__ __launch_bounds__(kRowsBlock) void case_select_fixed_kernel(const CaseSelectParams p) {
  CHQ_FOR_WAVE_ROWS(base, p.nrows) {
    const int64_t i = base + lane_id(), wave_end = wave_rows_end(p.nrows, base);
    bool valid = false;
    if (i < p.nrows) {
      const CaseBranch& b = p.br[case_choice(p.masks, p.words, p.n_when, i)];
      valid = case_branch_valid(b, i);
      uint8_t* out = (uint8_t*)p.out_values + i * W;
      if (valid) case_copy_value<W>(b, i, out);
      else {
        const CaseBranch zero{nullptr, nullptr, nullptr, 0, 0, 0, CASE_CONST, 0};
        case_copy_value<W>(zero, i, out);
      }
    }
    store_validity_word(p.out_validity, p.null_count, base, wave_end, __ballot(valid));
  }
}

__global__ __launch_bounds__(kRowsBlock) void case_rows_kernel(const CaseSelectParams p) {
  CHQ_FOR_WAVE_ROWS(base, p.nrows) {
    const int64_t i = base + lane_id(), wave_end = wave_rows_end(p.nrows, base);
    bool valid = false;
    if (i < p.nrows) {
      const CaseBranch& b = p.br[case_choice(p.masks, p.words, p.n_when, i)];
      valid = case_branch_valid(b, i);
      int32_t first = 0, len = 0;
      if (valid) case_string_range(b, i, &first, &len);
      p.out_len[i] = len;
    }
    store_validity_word(p.out_validity, p.null_count, base, wave_end, __ballot(valid));
  }
}

// Rows whose output is empty (null rows among them) read nothing.  out_offsets has nrows + 1 entries.
__global__ __launch_bounds__(kRowsBlock) void case_gather_kernel(const CaseSelectParams p) {
  CHQ_FOR_WAVE_ROWS(base, p.nrows) {
    const int64_t i = base + lane_id(), wave_end = wave_rows_end(p.nrows, base);
    int32_t ob = 0, n = 0;
    const uint8_t* src = nullptr;
    if (i < p.nrows) {
      ob = p.out_offsets[i];
      n = p.out_offsets[i + 1] - ob;
      if (n > 0) {   // (then the chosen branch is valid here: case_rows_kernel gave a null row 0 bytes)
        const CaseBranch& b = p.br[case_choice(p.masks, p.words, p.n_when, i)];
        int32_t first, len;
        case_string_range(b, i, &first, &len);
        src = b.data + first;
      }
    }
    copy_rows(wave_spans_more_than(p.out_offsets, base, wave_end, CASE_WAVE_MODE_BYTES), src, p.out_data, ob, n);
  }
}
}  // namespace

hipError_t launch_case_masks(const CaseMasksParams& p, hipStream_t stream) {
  hipLaunchKernelGGL(case_masks_kernel, dim3(rows_grid(p.words, 256 * 32)), dim3(256), 0, stream, p);
  return hipGetLastError();
}
hipError_t launch_case_and(const CaseAndParams& p, hipStream_t stream) {
  hipLaunchKernelGGL(case_and_kernel, dim3(rows_grid((p.nrows + 63) / 64, 256 * 32)), dim3(256), 0, stream, p);
  return hipGetLastError();
}
hipError_t launch_case_select_bool(const CaseSelectParams& p, hipStream_t stream) {
  hipLaunchKernelGGL(case_select_bool_kernel, dim3(rows_grid(p.words, 256 * 32)), dim3(256), 0, stream, p);
  return hipGetLastError();
}
hipError_t launch_case_select_fixed(const CaseSelectParams& p, hipStream_t stream) {
  const dim3 grid(rows_grid(p.nrows, 256 * 32)), block(256);
  switch (p.width) {
    case 1: hipLaunchKernelGGL(case_select_fixed_kernel<1>, grid, block, 0, stream, p); break;
    case 2: hipLaunchKernelGGL(case_select_fixed_kernel<2>, grid, block, 0, stream, p); break;
    case 4: hipLaunchKernelGGL(case_select_fixed_kernel<4>, grid, block, 0, stream, p); break;
    case 8: hipLaunchKernelGGL(case_select_fixed_kernel<8>, grid, block, 0, stream, p); break;
    case 16: hipLaunchKernelGGL(case_select_fixed_kernel<16>, grid, block, 0, stream, p); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}
hipError_t launch_case_rows(const CaseSelectParams& p, hipStream_t stream) {
  hipLaunchKernelGGL(case_rows_kernel, dim3(rows_grid(p.nrows, 256 * 32)), dim3(256), 0, stream, p);
  return hipGetLastError();
}
hipError_t launch_case_gather(const CaseSelectParams& p, hipStream_t stream) {
  hipLaunchKernelGGL(case_gather_kernel, dim3(rows_grid(p.nrows, 256 * 32)), dim3(256), 0, stream, p);
  return hipGetLastError();
}
}  // namespace chq
