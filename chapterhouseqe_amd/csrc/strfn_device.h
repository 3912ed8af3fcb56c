// strfn_device.h -- the scalar string functions (`||`, UPPER / LOWER, LENGTH, OCTET_LENGTH, SUBSTRING, TRIM): the per-row
// rules, shared by the host (constant folding in plan.cpp, the stand-alone sanitizer program of the tests) and the device
// (strfn.hip), and the parameter blocks of strfn.hip's kernels.  DESIGN.md section 3.12.
//
// Everything is bytewise.  Case and whitespace are ASCII only (a..z / A..Z, byte 0x20).  A CODE POINT START is a byte that
// is not 0x80..0xBF -- the definition `_` uses in LIKE.  Invalid UTF-8 is never an error and never makes a function read
// outside the row: its result is whatever these rules give.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CHQ_STRFN_HD __host__ __device__
#else
#define CHQ_STRFN_HD
#endif

namespace chq {

// `a || b || c` is flattened into one operation of up to this many parts; a longer chain nests.
constexpr int STRFN_MAX_PARTS = 8;
// strfn.hip picks its mode per wave like like.hip: when the 64 rows of a wave hold MORE than this many source bytes the wave
// walks them one row at a time, otherwise every lane takes its own row.  Untuned: LIKE's value, chosen before any measurement.
constexpr int STRFN_WAVE_MODE_BYTES = 4096;

enum StrFn : int32_t {
  STRFN_UPPER = 0, STRFN_LOWER, STRFN_LENGTH, STRFN_OCTET_LENGTH, STRFN_SUBSTRING, STRFN_TRIM, STRFN_LTRIM, STRFN_RTRIM, STRFN_CONCAT
};

// ---- the per-row rules ---------------------------------------------------------------------------------------------------
CHQ_STRFN_HD inline uint8_t strfn_map_byte(uint8_t b, bool upper) {
  if (upper) return (b >= 'a' && b <= 'z') ? (uint8_t)(b - 32) : b;
  return (b >= 'A' && b <= 'Z') ? (uint8_t)(b + 32) : b;
}
CHQ_STRFN_HD inline bool strfn_is_start(uint8_t b) { return (b & 0xC0) != 0x80; }

// LENGTH: code point starts in s[0, n)
CHQ_STRFN_HD inline int32_t strfn_count_starts(const uint8_t* s, int32_t n) {
  int32_t c = 0;
  for (int32_t i = 0; i < n; ++i) c += strfn_is_start(s[i]);
  return c;
}
// byte index of the k-th (1-based, k >= 1) code point start of s[0, n), or n when there are fewer
CHQ_STRFN_HD inline int32_t strfn_kth_start(const uint8_t* s, int32_t n, int64_t k) {
  for (int32_t i = 0; i < n; ++i)
    if (strfn_is_start(s[i]) && --k == 0) return i;
  return n;
}
// SUBSTRING(s FROM p [FOR cnt]), cnt >= 0: the bytes [*first, *first + *len) of s[0, n).  The window begins at byte 0 when
// p <= 1, else at the p-th start (or n); it ends at the max(p + cnt, 1)-th start (or n), at n without FOR.  With p <= 1 and
// no FOR the string is not read.  (max(.., 1) and not "byte 0 when p + cnt <= 1": on valid UTF-8 the first start IS byte 0,
// and on a row that begins with stray continuation bytes this keeps `from p for n` = `from 1 for max(0, p + n - 1)` for every
// p <= 0 -- both give those stray bytes.)
// (`kth(off, m, k)`: the k-th start of the m bytes at `off` of the row, as an index from `off` -- sequential here, by the
// whole wave in strfn.hip's wave-per-row mode; the window logic is the same)
template <class Kth>
CHQ_STRFN_HD inline void strfn_substr_window_with(const Kth& kth, int32_t n, int32_t p, bool has_cnt, int32_t cnt, int32_t* first, int32_t* len) {
  int32_t b, e;
  if (p <= 1) {
    b = 0;
    const int64_t k = (int64_t)p + cnt;
    e = has_cnt ? kth(0, n, k < 1 ? 1 : k) : n;
  } else {
    b = kth(0, n, (int64_t)p);
    // the byte at b is the p-th start: the (p + cnt)-th of the row is the (cnt + 1)-th from there
    e = (has_cnt && b < n) ? b + kth(b, n - b, (int64_t)cnt + 1) : n;
  }
  *first = b; *len = e - b;
}
struct StrfnSeqKth {
  const uint8_t* s;
  CHQ_STRFN_HD int32_t operator()(int32_t off, int32_t m, int64_t k) const { return m > 0 ? strfn_kth_start(s + off, m, k) : 0; }
};
CHQ_STRFN_HD inline void strfn_substr_window(const uint8_t* s, int32_t n, int32_t p, bool has_cnt, int32_t cnt, int32_t* first, int32_t* len) {
  strfn_substr_window_with(StrfnSeqKth{s}, n, p, has_cnt, cnt, first, len);
}
// TRIM / LTRIM / RTRIM: byte 0x20 only
CHQ_STRFN_HD inline void strfn_trim_window(const uint8_t* s, int32_t n, bool left, bool right, int32_t* first, int32_t* len) {
  int32_t b = 0, e = n;
  if (left) while (b < e && s[b] == 0x20) ++b;
  if (right) while (e > b && s[e - 1] == 0x20) --e;
  *first = b; *len = e - b;
}

// ---- strfn.hip -----------------------------------------------------------------------------------------------------------
// One operand: a Utf8 column (`offsets` at row 0 of the possibly sliced column, offsets[0] need not be 0; `data` may be null
// when every string is empty; `validity` a bitmap read from bit `validity_offset`, or null), or -- `offsets` null -- a
// literal of `lit_len` bytes at `data` (a small device buffer), the same for every row.
struct StrPart {
  const int32_t* offsets;
  const uint8_t* data;
  const void* validity; int64_t validity_offset;
  int32_t lit_len; int32_t pad;
};

// strfn_rows_kernel, one wave per 64 rows.  LENGTH / OCTET_LENGTH: `out_i32` = the values.  SUBSTRING / TRIM: `out_i32` =
// the byte length of each result row and `out_start` = where it begins in part[0].data (an index from data, not from the
// row).  CONCAT: `out_i32` = the summed lengths of the parts.  A null row (any part null) gets 0.  Validity and the
// zero-initialised null count as the kernels of typed_ops.hip write them: (nrows + 63) / 64 words, one atomic per wave.
struct StrRowsParams {
  StrPart part[STRFN_MAX_PARTS];
  int32_t n_parts; int32_t fn;          // StrFn
  int32_t p, cnt, has_cnt, pad;         // SUBSTRING
  int64_t nrows;
  int32_t* out_i32; int32_t* out_start;
  unsigned long long* out_validity; unsigned long long* null_count;
};

// The exclusive scan of the row lengths is launch_offsets_scan (scan.hip, typed_ops.h) over tiles of STRFN_SCAN_CHUNK rows,
// the total written behind the offsets.  The host checks the 64-bit total against the Int32 range before anything reads
// offsets that wrapped.  The lengths are read as UNSIGNED: a `||` row whose parts sum past 2^32 - 1 is stored as that, which
// alone puts the total out of range.
constexpr int STRFN_SCAN_CHUNK = 2048;

// strfn_gather_kernel: row i of the output = for each part, its bytes ([start[i], start[i] + length) of part[0].data when
// `start` is given: SUBSTRING / TRIM).  Rows whose output is empty (null rows among them) are not read.
struct StrGatherParams {
  StrPart part[STRFN_MAX_PARTS];
  int32_t n_parts; int32_t pad;
  int64_t nrows;
  const int32_t* start;
  const int32_t* out_offsets; uint8_t* out_data;
};

// strfn_bytemap_kernel: out[0, n) = map(in[0, n)), oblivious of rows.  Every load lies inside in[0, n).
struct StrByteMapParams { const uint8_t* in; uint8_t* out; int64_t n; int32_t upper; int32_t pad; };
// out[i] = in[i] - in[0], i in [0, n): the offsets of a length-preserving function (ipc.cpp has the same for its own use)
struct StrRebaseParams { const int32_t* in; int32_t* out; int64_t n; };

}  // namespace chq
