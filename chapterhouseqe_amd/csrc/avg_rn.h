// avg_rn.h -- round-to-nearest-even of an exact 128-bit integer total to binary64, for AVG over integers (aggregate_acc.h:
// AO_AVG_INT).  The device has no conversion from a 128-bit integer (no __floattidf), so it is written out in plain C++ and
// shared with the host, where a stand-alone program of the tests checks it under the sanitizers.  DESIGN.md section 3.7.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define CHQ_AVG_HD __host__ __device__
#else
#define CHQ_AVG_HD
#endif

namespace chq {

// index of the highest set bit of x (x != 0)
CHQ_AVG_HD inline int avg_top_bit(uint64_t x) {
  int p = 0;
  if (x >> 32) { x >>= 32; p += 32; }
  if (x >> 16) { x >>= 16; p += 16; }
  if (x >> 8) { x >>= 8; p += 8; }
  if (x >> 4) { x >>= 4; p += 4; }
  if (x >> 2) { x >>= 2; p += 2; }
  if (x >> 1) { p += 1; }
  return p;
}

// RN(T) for the total T = hi * 2^64 + lo, read as two's complement when `is_signed`, else as unsigned: the binary64 nearest
// to T, ties to even.  Every T of 128 bits is below 2^128 in magnitude, so the result is finite.
CHQ_AVG_HD inline double avg_rn128(uint64_t lo, uint64_t hi, bool is_signed) {
  // sign, then magnitude (-2^127 negates to 2^127, which the unsigned words hold)
  const bool neg = is_signed && (hi >> 63) != 0;
  if (neg) {
    lo = ~lo + 1;
    hi = ~hi + (lo == 0 ? 1 : 0);
  }
  if ((lo | hi) == 0) return 0.0;
  // normalise across the two words: p = position of the leading bit, 0..127
  const int p = hi ? 64 + avg_top_bit(hi) : avg_top_bit(lo);
  uint64_t mant;   // the 53 leading bits, the leading one at bit 52
  int e = p;
  if (p <= 52) {
    mant = lo << (52 - p);   // exact
  } else {
    const int s = p - 52;   // bits dropped: 1..75
    bool guard, sticky;
    if (s < 64) {
      mant = (lo >> s) | (hi ? hi << (64 - s) : 0);   // (hi != 0 only where s >= 12: the shift count stays below 64)
      guard = (lo >> (s - 1)) & 1;
      sticky = (lo & ((1ull << (s - 1)) - 1)) != 0;
    } else if (s == 64) {
      mant = hi;
      guard = lo >> 63;
      sticky = (lo & ~(1ull << 63)) != 0;
    } else {   // the leading bit is in the high word and so is the guard bit: the sticky bit sees the whole low word
      const int sh = s - 64;   // 1..11
      mant = hi >> sh;
      guard = (hi >> (sh - 1)) & 1;
      sticky = (hi & ((1ull << (sh - 1)) - 1)) != 0 || lo != 0;
    }
    if (guard && (sticky || (mant & 1))) {   // ties to even
      ++mant;
      if (mant >> 53) {   // the carry out of the mantissa: 2^53 -> 2^52, one exponent up
        mant >>= 1;
        ++e;
      }
    }
  }
  const uint64_t bits = ((uint64_t)neg << 63) | ((uint64_t)(e + 1023) << 52) | (mant & ((1ull << 52) - 1));
  double d;
  memcpy(&d, &bits, 8);
  return d;
}

}  // namespace chq
