// case_device.h -- searched CASE (and what types to it: simple CASE, COALESCE, NULLIF): the per-word and per-row rules, shared
// by the host (constant folding in plan.cpp, the stand-alone sanitizer program of the tests) and the device (case.hip), and
// the parameter blocks of case.hip's kernels.  DESIGN.md section 3.13.
//
// Row i takes the result of the first WHEN whose condition is TRUE AND VALID on that row, else the ELSE, else NULL.  The
// choice is kept as bitmaps aligned to bit 0 -- one TAKE mask per WHEN and the REMAINING mask behind them -- which are also
// the guards of the lazy-error rule: a result is evaluated under its take mask, a condition under the remaining mask of the
// WHENs before it.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CHQ_CASE_HD __host__ __device__
#else
#define CHQ_CASE_HD
#endif

namespace chq {

// WHENs of one operation; a longer CASE nests (WHEN 9 onward is a CASE in the ELSE slot)
constexpr int CASE_MAX_WHENS = 8;
// x IN (l1 .. lk): k in 1..CASE_MAX_IN_LIST (typed as a chain of `=`; plan.cpp)
constexpr int CASE_MAX_IN_LIST = 32;
// case_gather_kernel picks its mode per wave like strfn.hip: more than this many output bytes in the wave's 64 rows and the
// wave copies them one row at a time.  Untuned: the string functions' value, which was chosen before any measurement.
constexpr int CASE_WAVE_MODE_BYTES = 4096;

// ---- the per-word rules ----------------------------------------------------------------------------------------------------
// rows of word w of an nrows-row bitmap, as a mask
CHQ_CASE_HD inline uint64_t case_rows_mask(int64_t w, int64_t nrows) {
  const int64_t rows = nrows - 64 * w;
  return rows >= 64 ? ~0ull : rows <= 0 ? 0ull : ((1ull << rows) - 1);
}
// Word w of a bitmap that is read from bit `bit_off` of `bits`, re-aligned to bit 0; bits of rows >= nrows are 0.  Without a
// bitmap every row's bit is set.  Only the bytes that hold one of these rows' bits are loaded: the bitmap may end with them.
CHQ_CASE_HD inline uint64_t case_load_word(const uint8_t* bits, int64_t bit_off, int64_t w, int64_t nrows) {
  const uint64_t rm = case_rows_mask(w, nrows);
  if (!bits || !rm) return rm;
  const int64_t rows = nrows - 64 * w < 64 ? nrows - 64 * w : 64;
  const int64_t b0 = bit_off + 64 * w;
  const uint8_t* p = bits + (b0 >> 3);
  const int sh = (int)(b0 & 7);
  const int nbytes = (int)((sh + rows + 7) >> 3);   // 1..9
  uint64_t v = 0;
  for (int k = 0; k < nbytes && k < 8; ++k) v |= (uint64_t)p[k] << (8 * k);
  v >>= sh;
  if (nbytes == 9) v |= (uint64_t)p[8] << (64 - sh);   // (then sh > 0)
  return v & rm;
}
// one WHEN: the rows it takes, which leave `remaining`
CHQ_CASE_HD inline uint64_t case_take(uint64_t* remaining, uint64_t cond, uint64_t valid) {
  const uint64_t t = *remaining & cond & valid;
  *remaining &= ~t;
  return t;
}

// ---- parameter blocks --------------------------------------------------------------------------------------------------------
enum CaseSrc : int32_t { CASE_COLUMN = 0, CASE_CONST = 1, CASE_NULL = 2 };

// One condition: a Boolean column (`values` / `validity` bitmaps read from bit `offset`; validity may be null), a constant
// (`const_val` 0 / 1) or NULL.
struct CaseCond {
  const uint8_t* values; const uint8_t* validity;
  int64_t offset;
  int32_t kind; int32_t const_val;
};
// case_masks_kernel, one lane per 64 rows: for WHENs [first, first + n) writes take_k to masks[k * words ..] and the remaining
// mask to masks[n_total * words ..], which it reads first when first > 0 (every row remains otherwise).
struct CaseMasksParams {
  CaseCond cond[CASE_MAX_WHENS];   // cond[j] = WHEN first + j
  int32_t first, n, n_total, pad;
  int64_t nrows, words;
  unsigned long long* masks;       // [(n_total + 1) * words]
};
// case_and_kernel: out[w] = word w of `bits` read from `bit_off` (all rows without one) AND guard[w] (all rows without one):
// the validity of a guarded view, or a bitmap re-aligned to bit 0.
struct CaseAndParams { const uint8_t* bits; int64_t bit_off; const unsigned long long* guard; int64_t nrows; unsigned long long* out; };

// One result (THEN / ELSE): a column -- `values` at row 0 of the possibly sliced column for fixed widths and Utf8 (the Int32
// offsets; `data` the bytes), the bitmap read from bit `offset` for Boolean; `validity` read from bit `offset`, or null --, a
// constant (`const_lo` / `const_hi`: the value bits; Utf8: `lit_len` bytes at `data`) or NULL.
struct CaseBranch {
  const uint8_t* values; const uint8_t* data; const uint8_t* validity;
  int64_t offset;
  uint64_t const_lo, const_hi;
  int32_t kind; int32_t lit_len;
};
// The select kernels.  br[k] = the result of WHEN k, br[n_when] = the ELSE (CASE_NULL without one).  `masks` as
// case_masks_kernel left them.  out_validity: (nrows + 63) / 64 words; null_count zero-initialised.
//   case_select_bool_kernel   out_values = the result bitmap, word-wise
//   case_select_fixed_kernel  out_values = nrows values of `width` bytes (a null row's value is 0)
//   case_rows_kernel          out_len = the byte length of every row's chosen string (a null row: 0)
//   case_gather_kernel        out_data[out_offsets[i] ..] = the bytes of row i's chosen string
struct CaseSelectParams {
  CaseBranch br[CASE_MAX_WHENS + 1];
  int32_t n_when, width;
  int64_t nrows, words;
  const unsigned long long* masks;
  void* out_values; unsigned long long* out_validity; unsigned long long* null_count;
  int32_t* out_len; const int32_t* out_offsets; uint8_t* out_data;
};

// ---- the per-row rules -------------------------------------------------------------------------------------------------------
// the branch row i takes: k < n_when = WHEN k, n_when = the ELSE slot
CHQ_CASE_HD inline int case_choice(const unsigned long long* masks, int64_t words, int n_when, int64_t i) {
  const int64_t w = i >> 6;
  const int b = (int)(i & 63);
  for (int k = 0; k < n_when; ++k)
    if ((masks[(int64_t)k * words + w] >> b) & 1) return k;
  return n_when;
}
CHQ_CASE_HD inline bool case_branch_valid(const CaseBranch& b, int64_t i) {
  if (b.kind != CASE_COLUMN) return b.kind == CASE_CONST;
  if (!b.validity) return true;
  const int64_t pos = b.offset + i;
  return (b.validity[pos >> 3] >> (pos & 7)) & 1;
}
// the W-byte value of row i of a branch that is valid there, to `out` (W-aligned; the source of 8 and 16 bytes is read in
// 4-byte words: Arrow guarantees its buffers' 8-byte alignment only through their producer)
template <int W>
CHQ_CASE_HD inline void case_copy_value(const CaseBranch& b, int64_t i, uint8_t* out) {
  if (W >= 8) {
    uint32_t* o = (uint32_t*)out;
    if (b.kind == CASE_CONST) {
      o[0] = (uint32_t)b.const_lo; o[1] = (uint32_t)(b.const_lo >> 32);
      if (W == 16) { o[2] = (uint32_t)b.const_hi; o[3] = (uint32_t)(b.const_hi >> 32); }
    } else {
      const uint32_t* s = (const uint32_t*)b.values + (W / 4) * i;
      for (int k = 0; k < W / 4; ++k) o[k] = s[k];
    }
  } else if (W == 4) {
    *(uint32_t*)out = b.kind == CASE_CONST ? (uint32_t)b.const_lo : ((const uint32_t*)b.values)[i];
  } else if (W == 2) {
    *(uint16_t*)out = b.kind == CASE_CONST ? (uint16_t)b.const_lo : ((const uint16_t*)b.values)[i];
  } else {
    *out = b.kind == CASE_CONST ? (uint8_t)b.const_lo : b.values[i];
  }
}
// the bytes [*first, *first + *len) of b.data that are row i's string in a branch that is valid there
CHQ_CASE_HD inline void case_string_range(const CaseBranch& b, int64_t i, int32_t* first, int32_t* len) {
  if (b.kind == CASE_CONST) { *first = 0; *len = b.lit_len; return; }
  const int32_t* offs = (const int32_t*)b.values;
  *first = offs[i]; *len = offs[i + 1] - offs[i];
}
// one word of a Boolean result: its values and its validity from the masks and the branches' words
CHQ_CASE_HD inline void case_select_bool_word(const CaseSelectParams& p, int64_t w, uint64_t* out_val, uint64_t* out_valid) {
  uint64_t val = 0, valid = 0;
  for (int k = 0; k <= p.n_when; ++k) {
    const uint64_t m = p.masks[(int64_t)k * p.words + w];
    const CaseBranch& b = p.br[k];
    if (!m || b.kind == CASE_NULL) continue;
    if (b.kind == CASE_CONST) { valid |= m; if (b.const_lo & 1) val |= m; continue; }
    const uint64_t bv = case_load_word(b.validity, b.offset, w, p.nrows);
    valid |= m & bv;
    val |= m & bv & case_load_word(b.values, b.offset, w, p.nrows);
  }
  *out_val = val; *out_valid = valid;
}

}  // namespace chq
