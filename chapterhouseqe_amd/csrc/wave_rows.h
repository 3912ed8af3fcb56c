// wave_rows.h -- device side only (.hip files include it): the row-wise scheme of the typed operations (typed_ops.hip, like.hip,
// strfn.hip, case.hip, cast.hip).  A wave owns 64 consecutive rows, so a word of an output bitmap is
// one ballot, stored whole by lane 0 and never with an atomic, and the wave's nulls are its row count less one popcount: at
// most one atomic per wave.  The launched grid is capped (rows_grid, typed_ops.h), the rows behind it are walked in rounds.
#pragma once
#include "scan_device.h"   // lane_id, bit_at

namespace chq {

constexpr int kRowsBlock = 256;   // threads of a workgroup of every kernel on this scheme

// The row loop: `base` is the first of the 64 consecutive rows this wave owns in this round, [base, wave_rows_end(nrows, base)).
// The loop condition is wave-uniform, so the whole wave is converged in the body and ballots and shuffles are legal there.  Lane l
// takes row i = base + l; a lane with i >= nrows takes part too -- the ballots need it -- and the body guards its loads and
// stores with i < nrows: no offset of a row >= nrows is read (offsets[wave_rows_end] is the last one a body may touch).
// (A macro, like the grid-stride loop macros of other code bases: the body stays in the kernel, which reads its parameter block
// directly.  As a function template over a lambda the same loop compiled to slower code: profiles/typed_rows_refactor/.)
#define CHQ_FOR_WAVE_ROWS(base, nrows) \
  for (int64_t base = ((int64_t)blockIdx.x * kRowsBlock + threadIdx.x) & ~63LL; base < (nrows); base += (int64_t)gridDim.x * kRowsBlock)
__device__ __forceinline__ int64_t wave_rows_end(int64_t nrows, int64_t base) { return nrows - base < 64 ? nrows : base + 64; }

// row i of an input whose validity bitmap is read from bit `bit_offset` (a sliced view); no bitmap = no nulls
__device__ __forceinline__ bool row_valid(const void* validity, int64_t bit_offset, int64_t i) {
  return !validity || bit_at(validity, bit_offset + i);
}

// vm = the ballot of the valid rows of [base, wave_end): lane 0 stores the wave's validity word, and one atomic adds the wave's
// nulls.  (cast.hip counts its nulls in a pass of its own and writes the word next to its failure flag.)
__device__ __forceinline__ void store_validity_word(unsigned long long* out_validity, unsigned long long* null_count, int64_t base,
                                                    int64_t wave_end, uint64_t vm) {
  if (lane_id() == 0) {
    out_validity[base >> 6] = vm;
    const unsigned nulls = (unsigned)(wave_end - base) - (unsigned)__popcll(vm);
    if (nulls) atomicAdd(null_count, (unsigned long long)nulls);
  }
}
// the same for a kernel with a lane per 64-row WORD: `nulls` is per lane, summed over the wave, added by one lane
__device__ __forceinline__ void add_nulls(unsigned long long* null_count, unsigned nulls) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) nulls += __shfl_xor(nulls, o, 64);
  if (lane_id() == 0 && nulls) atomicAdd(null_count, (unsigned long long)nulls);
}

// The mode of a wave over Utf8 rows, decided by the wave itself: do its rows span more than `bytes` (the operator's
// *_WAVE_MODE_BYTES)?  Then the wave takes its rows one after the other, 64 bytes per step; otherwise a lane takes a row.
__device__ __forceinline__ bool wave_spans_more_than(const int32_t* offsets, int64_t base, int64_t wave_end, int32_t bytes) {
  return (int64_t)offsets[wave_end] - (int64_t)offsets[base] > bytes;
}

// Every lane copies the n bytes at src to out_data + ob (n = 0, src unset: a lane without a row).  wave_mode (wave-uniform):
// the non-empty rows are taken in turn, their source, destination and length shuffled from the owning lane, lane l copying
// bytes l, l + 64, ...
__device__ __forceinline__ void copy_rows(bool wave_mode, const uint8_t* src, uint8_t* out_data, int32_t ob, int32_t n) {
  if (wave_mode) {
    for (uint64_t todo = __ballot(n > 0); todo; todo &= todo - 1) {
      const int row = __ffsll((long long)todo) - 1;
      const uint8_t* s = (const uint8_t*)__shfl((unsigned long long)(uintptr_t)src, row);
      uint8_t* dst = out_data + __shfl(ob, row);
      const int32_t rn = __shfl(n, row);
      for (int32_t j = lane_id(); j < rn; j += 64) dst[j] = s[j];
    }
  } else {
    uint8_t* dst = out_data + ob;
    for (int32_t j = 0; j < n; ++j) dst[j] = src[j];
  }
}

}  // namespace chq
