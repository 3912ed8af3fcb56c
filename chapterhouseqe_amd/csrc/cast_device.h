// cast_device.h -- CAST / TRY_CAST: the per-row rules, shared by the host (constant folding in
// plan.cpp, the stand-alone sanitizer program of the tests) and the device (cast.hip), and the parameter blocks of cast.hip's
// kernels.
//
// Every value travels as 64 bits: a signed integer sign-extended, an unsigned one zero-extended, a Boolean 0 / 1, a float its
// IEEE bit pattern in the low 16 / 32 / 64 bits.  The float conversions are integer arithmetic on those patterns, so the host
// and the device give the same bits whatever the denormal mode or the compiler's lowering of a 64-bit convert is:
//   integer -> Float16 / 32 / 64   the magnitude IS the significand (cast_round_pack): no intermediate, one rounding
//   float   -> float               the source's significand and exponent, rounded once to the target (cast_float_bits)
//   float   -> integer             the pattern widened EXACTLY to Float64 (every Float16 / Float32 value is one), then
//                                  truncated toward zero and range-checked against powers of two, which Float64 holds exactly
// A NaN keeps its sign and the top payload bits that fit, with the quiet bit set (tests/float_reference.py: convert_float).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CHQ_CAST_HD __host__ __device__
#else
#define CHQ_CAST_HD
#endif

namespace chq {

// The types of a cast, numbered like DType (device_program.h), which a plain C++ program does not include.
enum CastType : int32_t {
  CT_BOOL = 0, CT_I8, CT_I16, CT_I32, CT_I64, CT_U8, CT_U16, CT_U32, CT_U64, CT_F16, CT_F32, CT_F64, CT_UTF8
};
CHQ_CAST_HD inline bool cast_is_int(int t) { return t >= CT_I8 && t <= CT_U64; }
CHQ_CAST_HD inline bool cast_is_signed(int t) { return t >= CT_I8 && t <= CT_I64; }
CHQ_CAST_HD inline bool cast_is_float(int t) { return t >= CT_F16 && t <= CT_F64; }
// value bits of an integer type: 8, 16, 32, 64
CHQ_CAST_HD inline int cast_int_bits(int t) { return 8 << ((t - CT_I8) & 3); }
// bytes of a fixed-width value (Boolean and Utf8: 0)
CHQ_CAST_HD inline int cast_width(int t) {
  if (cast_is_int(t)) return cast_int_bits(t) >> 3;
  return t == CT_F16 ? 2 : t == CT_F32 ? 4 : t == CT_F64 ? 8 : 0;
}
// explicit mantissa / exponent bits of a float type
CHQ_CAST_HD inline int cast_mbits(int t) { return t == CT_F16 ? 10 : t == CT_F32 ? 23 : 52; }
CHQ_CAST_HD inline int cast_ebits(int t) { return t == CT_F16 ? 5 : t == CT_F32 ? 8 : 11; }

// the largest magnitude a target holds on the positive / the negative side
CHQ_CAST_HD inline uint64_t cast_max_pos(int to) {
  const int b = cast_int_bits(to);
  return cast_is_signed(to) ? (1ull << (b - 1)) - 1 : (b == 64 ? ~0ull : (1ull << b) - 1);
}
CHQ_CAST_HD inline uint64_t cast_max_neg(int to) { return cast_is_signed(to) ? 1ull << (cast_int_bits(to) - 1) : 0; }

// ---- integer -> integer: value preserved, fails outside the target's range ----------------------------------------------
CHQ_CAST_HD inline bool cast_int_to_int(uint64_t bits, bool from_signed, int to, uint64_t* out) {
  const bool neg = from_signed && (int64_t)bits < 0;
  const uint64_t mag = neg ? 0 - bits : bits;
  if (mag > (neg ? cast_max_neg(to) : cast_max_pos(to))) return false;
  *out = bits;   // (two's complement: the low bytes of the sign- or zero-extended pattern are the target's value)
  return true;
}

// ---- (-1)^neg * sig * 2^e2, sig != 0, rounded once to nearest even into a float of mbits / ebits -----------------------
// Overflow gives infinity, a result below the smallest normal is a subnormal (or zero).  The quotient q carries the implicit
// bit of a normal number: adding it to (biased exponent - 1) << mbits also handles the carry into the next binade and a
// subnormal that rounds up to the smallest normal.
CHQ_CAST_HD inline uint64_t cast_round_pack(bool neg, uint64_t sig, int e2, int mbits, int ebits) {
  const int bias = (1 << (ebits - 1)) - 1;
  const uint64_t sign = neg ? 1ull << (mbits + ebits) : 0, inf = ((1ull << ebits) - 1) << mbits;
  const int top = 63 - __builtin_clzll(sig);
  const int biased = top + e2 + bias;                        // exponent field of a normal result
  const int shift = top - mbits + (biased < 1 ? 1 - biased : 0);   // bits of sig below the result's last place
  uint64_t q;
  if (shift <= 0) {
    q = sig << -shift;   // exact
  } else if (shift > top + 1) {
    q = 0;               // below half of the smallest subnormal
  } else if (shift == 64) {
    q = sig > (1ull << 63) ? 1 : 0;   // (top = 63: the half is 2^63, a tie goes to the even 0)
  } else {
    q = sig >> shift;
    const uint64_t rem = sig & ((1ull << shift) - 1), half = 1ull << (shift - 1);
    if (rem > half || (rem == half && (q & 1))) ++q;
  }
  const uint64_t mag = ((uint64_t)(biased < 1 ? 0 : biased - 1) << mbits) + q;
  return sign | (mag > inf ? inf : mag);
}

// ---- integer -> float: never fails -------------------------------------------------------------------------------------------
CHQ_CAST_HD inline uint64_t cast_int_to_float(uint64_t bits, bool from_signed, int to) {
  const bool neg = from_signed && (int64_t)bits < 0;
  const uint64_t mag = neg ? 0 - bits : bits;
  if (mag == 0) return 0;   // an integer zero is +0.0
  return cast_round_pack(neg, mag, 0, cast_mbits(to), cast_ebits(to));
}

// ---- float -> float: never fails ---------------------------------------------------------------------------------------------
CHQ_CAST_HD inline uint64_t cast_float_bits(uint64_t b, int from, int to) {
  const int sm = cast_mbits(from), se = cast_ebits(from), dm = cast_mbits(to), de = cast_ebits(to);
  const bool neg = (b >> (sm + se)) & 1;
  const int exp = (int)((b >> sm) & ((1ull << se) - 1));
  const uint64_t man = b & ((1ull << sm) - 1);
  const uint64_t sign = neg ? 1ull << (dm + de) : 0, inf = ((1ull << de) - 1) << dm;
  if (exp == (1 << se) - 1) {
    if (man == 0) return sign | inf;
    const uint64_t m = dm >= sm ? man << (dm - sm) : man >> (sm - dm);
    return sign | inf | m | (1ull << (dm - 1));
  }
  if (exp == 0 && man == 0) return sign;
  const int sbias = (1 << (se - 1)) - 1;
  // value = sig * 2^e2 with sig the integer significand
  const uint64_t sig = exp == 0 ? man : man | (1ull << sm);
  const int e2 = (exp == 0 ? 1 : exp) - sbias - sm;
  return cast_round_pack(neg, sig, e2, dm, de);
}

// ---- float -> integer: NaN and +-inf fail; else truncate toward zero; fails when the truncated value is out of range ---
CHQ_CAST_HD inline bool cast_float_to_int(uint64_t b, int from, int to, uint64_t* out) {
  const uint64_t d = from == CT_F64 ? b : cast_float_bits(b, from, CT_F64);   // exact
  if (((d >> 52) & 0x7ff) == 0x7ff) return false;
  double x;
  __builtin_memcpy(&x, &d, 8);
  const double t = __builtin_trunc(x);   // (-0.9 -> -0.0, which is inside every range and converts to 0)
  const int bits = cast_int_bits(to);
  // 2^(bits - 1) and 2^bits as Float64, built from their exponents
  const uint64_t hi_bits = (uint64_t)(1023 + (cast_is_signed(to) ? bits - 1 : bits)) << 52;
  double hi;
  __builtin_memcpy(&hi, &hi_bits, 8);
  if (cast_is_signed(to)) {
    if (!(t >= -hi && t < hi)) return false;
    *out = (uint64_t)(int64_t)t;
  } else {
    if (!(t >= 0.0 && t < hi)) return false;
    *out = (uint64_t)t;
  }
  return true;
}

// ---- numeric -> Boolean: x != 0 (NaN -> true, -0.0 -> false) ---------------------------------------------------------------
CHQ_CAST_HD inline bool cast_to_bool(uint64_t bits, int from) {
  if (cast_is_float(from)) return (bits & ((1ull << (cast_mbits(from) + cast_ebits(from))) - 1)) != 0;
  return bits != 0;
}

// One fixed-width value (Boolean, integer, float) to another fixed-width type.  False: the row fails.
CHQ_CAST_HD inline bool cast_fixed_value(uint64_t bits, int from, int to, uint64_t* out) {
  if (to == CT_BOOL) { *out = cast_to_bool(bits, from) ? 1 : 0; return true; }
  if (from == CT_BOOL) {   // 1 / 0, 1.0 / 0.0
    *out = cast_is_float(to) ? cast_int_to_float(bits & 1, false, to) : (bits & 1);
    return true;
  }
  if (cast_is_int(from)) {
    if (cast_is_int(to)) return cast_int_to_int(bits, cast_is_signed(from), to, out);
    *out = cast_int_to_float(bits, cast_is_signed(from), to);
    return true;
  }
  if (cast_is_int(to)) return cast_float_to_int(bits, from, to, out);
  *out = cast_float_bits(bits, from, to);
  return true;
}
// can a row of `from` fail on its way to `to`?  (What makes a CAST count as data-dependent for the lazy-error rule.)
CHQ_CAST_HD inline bool cast_can_fail(int from, int to) {
  if (from == CT_UTF8) return to != CT_UTF8;
  if (!cast_is_int(to) || from == CT_BOOL) return false;
  if (cast_is_float(from)) return true;
  // integer -> integer: unless the target holds the source's whole range
  const uint64_t src_pos = cast_max_pos(from), src_neg = cast_max_neg(from);
  return src_pos > cast_max_pos(to) || src_neg > cast_max_neg(to);
}

// ---- Utf8 -> integer: the whole row is [+-]?[0-9]+ ('-' only for signed targets), any number of leading zeros, no white
// space; the value must fit.  Reads s[0, n) only.
CHQ_CAST_HD inline bool cast_parse_int(const uint8_t* s, int32_t n, int to, uint64_t* out) {
  if (n <= 0) return false;
  int32_t i = 0;
  bool neg = false;
  if (s[0] == '+') i = 1;
  else if (s[0] == '-') { if (!cast_is_signed(to)) return false; neg = true; i = 1; }
  if (i == n) return false;
  const uint64_t limit = neg ? cast_max_neg(to) : cast_max_pos(to);
  uint64_t v = 0;
  for (; i < n; ++i) {
    const uint32_t d = (uint32_t)s[i] - '0';
    if (d > 9) return false;
    if (v > (limit - d) / 10) return false;   // v * 10 + d > limit (limit >= 127 > d)
    v = v * 10 + d;
  }
  *out = neg ? 0 - v : v;
  return true;
}

// ---- integer -> Utf8: shortest decimal, '-' for negatives: 1 to 20 bytes --------------------------------------------------
CHQ_CAST_HD inline int32_t cast_decimal_len(uint64_t bits, bool from_signed) {
  const bool neg = from_signed && (int64_t)bits < 0;
  uint64_t mag = neg ? 0 - bits : bits;
  int32_t n = neg ? 2 : 1;
  while (mag >= 10) { mag /= 10; ++n; }
  return n;
}
// writes the cast_decimal_len(bits, from_signed) = n bytes at dst
CHQ_CAST_HD inline void cast_write_decimal(uint64_t bits, bool from_signed, uint8_t* dst, int32_t n) {
  const bool neg = from_signed && (int64_t)bits < 0;
  uint64_t mag = neg ? 0 - bits : bits;
  for (int32_t k = n - 1; k >= (neg ? 1 : 0); --k) { dst[k] = (uint8_t)('0' + mag % 10); mag /= 10; }
  if (neg) dst[0] = '-';
}
// Boolean -> Utf8: `true` / `false`
CHQ_CAST_HD inline int32_t cast_bool_len(bool v) { return v ? 4 : 5; }
CHQ_CAST_HD inline void cast_write_bool(bool v, uint8_t* dst) {
  const char* w = v ? "true" : "false";
  for (int32_t k = 0; k < (v ? 4 : 5); ++k) dst[k] = (uint8_t)w[k];
}

// ---- cast.hip ----------------------------------------------------------------------------------------------------------------
// The kernels take a wave per 64 rows in a loop over rounds of a capped grid: CAST_GRID_CAP workgroups of 256 threads, so
// the second round begins at row CAST_GRID_CAP * 256.  A word of an output bitmap (validity, Boolean values) is the ballot
// of its wave, stored whole by one lane: no atomics.  `fail` is one zero-initialised word: a wave in which a VALID row fails
// stores 1 (CAST reads it back; TRY_CAST passes try_cast = 1 and such rows become null instead).
constexpr int CAST_GRID_CAP = 256 * 16;
constexpr int CAST_BLOCK = 256;

// cast_fixed_kernel: Boolean / integer / float -> Boolean / integer / float.  `values`: the values buffer at row 0 (a
// Boolean source: the bitmap, read from bit `values_offset`).  `validity` (or null) is read from bit `validity_offset`.
// out_validity[(nrows + 63) / 64] = input validity AND the row converted; rows that are null come out as 0.
struct CastFixedParams {
  const void* values; int64_t values_offset;
  const void* validity; int64_t validity_offset;
  int64_t nrows;
  int32_t from, to, try_cast, pad;   // CastType
  void* out_values;                  // fixed width: nrows values; Boolean: (nrows + 63) / 64 words
  unsigned long long* out_validity;
  uint32_t* fail;
};
// cast_parse_kernel: Utf8 -> integer, a lane per row.  Only the bytes [offsets[i], offsets[i + 1]) of a VALID row are read.
struct CastParseParams {
  const int32_t* offsets; const uint8_t* data;
  const void* validity; int64_t validity_offset;
  int64_t nrows;
  int32_t to, try_cast;
  void* out_values;
  unsigned long long* out_validity;
  uint32_t* fail;
};
// cast_len_kernel / cast_write_kernel: integer / Boolean -> Utf8.  The length kernel writes the byte length of every row
// (0 for a null row) and the validity words; launch_offsets_scan turns the lengths into offsets; the write kernel writes
// the bytes of row i at out_data + out_offsets[i].
struct CastPrintParams {
  const void* values; int64_t values_offset;
  const void* validity; int64_t validity_offset;
  int64_t nrows;
  int32_t from, pad;
  uint32_t* out_len;
  unsigned long long* out_validity;
  const int32_t* out_offsets; uint8_t* out_data;
};

}  // namespace chq
