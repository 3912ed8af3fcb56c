// like_device.h -- SQL LIKE: the compiled pattern and the ONE matcher, shared by the host (constant folding in plan.cpp,
// the stand-alone sanitizer program of the tests) and the device (like.hip).  DESIGN.md section 3.11.
//
// A pattern is compiled once on the host into ELEMENTS: a literal byte, or "one UTF-8 code point" (`_`).  `%` is not an
// element: it splits the elements into PIECES (runs of `%` collapse), and a piece always consumes a fixed number of code
// points.  The first piece is anchored at the start of the string and the last one at its end (each is empty when the
// pattern starts / ends with `%`); every piece in between goes at its LEFTMOST match at or after the current position,
// which is sufficient exactly because a piece has a fixed width in code points.  A pattern without `%` is one piece
// anchored at both ends.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CHQ_LIKE_HD __host__ __device__
#else
#define CHQ_LIKE_HD
#endif

namespace chq {

// Bound of a compiled pattern: elements (literal bytes + `_`) after escapes are resolved and `%` removed.  The pattern is a
// kernel argument (264 bytes).  Longer patterns: CHQ_ERR_NOT_SUPPORTED naming this bound.
constexpr int LIKE_MAX_ELEMS = 128;
// like.hip picks its mode per wave: when the 64 rows of a wave hold MORE than this many string bytes, the wave walks them
// one row at a time with one candidate position per lane; otherwise every lane matches its own row.  Untuned: 64 bytes per
// row on average, chosen before any measurement.
constexpr int LIKE_WAVE_MODE_BYTES = 4096;

constexpr uint8_t LIKE_ANY = 1;     // kind: the element is `_`, one code point (else: the literal byte in `byte`)
constexpr uint8_t LIKE_START = 2;   // kind: the element is the first of a piece that follows a `%`

struct LikePattern {
  uint8_t byte[LIKE_MAX_ELEMS];
  uint8_t kind[LIKE_MAX_ELEMS];
  int16_t n_elem;       // elements in all
  int16_t first_end;    // the piece anchored at the start is [0, first_end)           (empty: the pattern starts with `%`)
  int16_t last_begin;   // the piece anchored at the end is [last_begin, n_elem)       (empty: the pattern ends with `%`)
  int16_t has_pct;      // 0: no `%` at all, one piece anchored at both ends ([0, n_elem) = the first piece)
};

CHQ_LIKE_HD inline bool like_is_cont(uint8_t b) { return (b & 0xC0) == 0x80; }

// Elements [eb, ee) against s[p ..) where the string ends at `limit`: the position after the piece, or -1.  `_` takes one
// non-continuation byte and the continuation bytes 0x80..0xBF behind it.  Reads s[p .. limit) only.
CHQ_LIKE_HD inline int32_t like_piece_at(const LikePattern& pat, int eb, int ee, const uint8_t* s, int32_t p, int32_t limit) {
  for (int k = eb; k < ee; ++k) {
    if (p >= limit) return -1;
    const uint8_t c = s[p];
    if (pat.kind[k] & LIKE_ANY) {
      if (like_is_cont(c)) return -1;
      ++p;
      while (p < limit && like_is_cont(s[p])) ++p;
    } else {
      if (c != pat.byte[k]) return -1;
      ++p;
    }
  }
  return p;
}

// end of the piece that starts at element eb (middle pieces only: stops at last_begin)
CHQ_LIKE_HD inline int like_piece_end(const LikePattern& pat, int eb) {
  int e = eb + 1;
  while (e < pat.last_begin && !(pat.kind[e] & LIKE_START)) ++e;
  return e;
}

// The two anchored pieces.  False: no match.  True: the pieces in between must be found in s[*pos, *lim), in order.  (A
// pattern without `%` is decided here: then *pos == *lim on success and there is nothing in between.)
CHQ_LIKE_HD inline bool like_ends(const LikePattern& pat, const uint8_t* s, int32_t n, int32_t* pos, int32_t* lim) {
  if (!pat.has_pct) {
    const int32_t e = like_piece_at(pat, 0, pat.n_elem, s, 0, n);
    *pos = *lim = n;
    return e == n;
  }
  const int32_t p = like_piece_at(pat, 0, pat.first_end, s, 0, n);
  if (p < 0) return false;
  // step back over as many code points as the last piece takes: a `_`, or a literal byte that starts a character
  int32_t q = n;
  for (int k = pat.last_begin; k < pat.n_elem; ++k) {
    if (!(pat.kind[k] & LIKE_ANY) && like_is_cont(pat.byte[k])) continue;
    if (q <= p) return false;
    --q;
    while (q > p && like_is_cont(s[q])) --q;
  }
  if (like_piece_at(pat, pat.last_begin, pat.n_elem, s, q, n) != n) return false;
  *pos = p; *lim = q;
  return true;
}

// the whole match of one string, sequentially: what a lane does for its row, and what the host folds literals with
CHQ_LIKE_HD inline bool like_match(const LikePattern& pat, const uint8_t* s, int32_t n) {
  int32_t pos, lim;
  if (!like_ends(pat, s, n, &pos, &lim)) return false;
  for (int eb = pat.first_end; eb < pat.last_begin;) {
    const int ee = like_piece_end(pat, eb);
    int32_t e = -1;
    for (; pos + (ee - eb) <= lim; ++pos)   // (an element takes at least one byte)
      if ((e = like_piece_at(pat, eb, ee, s, pos, lim)) >= 0) break;
    if (e < 0) return false;
    pos = e;
    eb = ee;
  }
  return true;
}

// ---- compilation (host) ------------------------------------------------------------------------------------------------
enum LikeCompileStatus { LIKE_OK = 0, LIKE_TRAILING_ESCAPE, LIKE_TOO_LONG };

// `escape`: -1 for none, else one ASCII byte; the byte behind it is literal whatever it is
inline LikeCompileStatus like_compile(const uint8_t* text, int64_t len, int escape, LikePattern* out) {
  LikePattern p{};
  int n = 0;
  bool after_pct = false, lead_pct = false;
  for (int64_t i = 0; i < len; ++i) {
    uint8_t c = text[i], kind = 0;
    if (escape >= 0 && c == (uint8_t)escape) {
      if (i + 1 >= len) return LIKE_TRAILING_ESCAPE;
      c = text[++i];
    } else if (c == '%') {
      if (n == 0) lead_pct = true;
      after_pct = true;
      p.has_pct = 1;
      continue;
    } else if (c == '_') {
      kind = LIKE_ANY;
    }
    if (n >= LIKE_MAX_ELEMS) return LIKE_TOO_LONG;
    if (after_pct) kind |= LIKE_START;
    after_pct = false;
    p.byte[n] = c; p.kind[n] = kind;
    ++n;
  }
  p.n_elem = p.first_end = p.last_begin = (int16_t)n;
  if (p.has_pct) {
    if (lead_pct) p.first_end = 0;
    else for (int k = n - 1; k >= 0; --k) if (p.kind[k] & LIKE_START) p.first_end = (int16_t)k;
    if (!after_pct)   // the pattern does not end with `%`: the last piece starts behind the last `%`
      for (int k = 0; k < n; ++k) if (p.kind[k] & LIKE_START) p.last_begin = (int16_t)k;
  }
  *out = p;
  return LIKE_OK;
}

// like.hip: `offsets` at row 0 of the (possibly sliced) column, offsets[0] need not be 0; `data` may be null when every
// string is empty; `validity` a bitmap read from bit `validity_offset`, or null.  Output like the kernels of typed_ops.hip:
// (nrows + 63) / 64 value and validity words, bit i = row i, and the zero-initialised null count.
struct LikeParams {
  const int32_t* offsets;
  const uint8_t* data;
  const void* validity; int64_t validity_offset;
  int64_t nrows;
  unsigned long long* out_bits; unsigned long long* out_validity;
  unsigned long long* null_count;
  int32_t negated;   // NOT LIKE: the complement on valid rows
  int32_t pad;
  LikePattern pat;
};

}  // namespace chq
