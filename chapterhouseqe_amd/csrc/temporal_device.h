// temporal_device.h -- DATE / TIMESTAMP literals, EXTRACT / date_part and date_trunc: the per-row
// rules, shared by the host (the literal conversion of plan.cpp, the stand-alone sanitizer program of the tests) and the device
// (temporal.hip), and the parameter block of temporal.hip's kernels.
//
// A value is the raw integer of its Arrow column: Int32 days (Date32), Int64 milliseconds (Date64, read like Timestamp(ms)),
// Int64 units since 1970-01-01T00:00:00 (Timestamp), Int32 / Int64 units since midnight (Time32 / Time64).  It is split by
// FLOOR division into a day number and a time of day, so -1 s is 1969-12-31 23:59:59.  The calendar is the proleptic Gregorian
// one, computed from the day number with the era arithmetic of Hinnant's `civil_from_days`: no table, no branch on data.
// gfx950 has no integer divide: every divisor below is a compile-time constant of its instantiation (the source kind is a
// template parameter).  The first split is 64-bit; behind the range check the day number fits 32 bits and the calendar runs in
// 32 bits.  The time of day fits 32 bits for seconds and milliseconds; for microseconds and nanoseconds the clock fields and the
// sub-day truncations take one more 64-bit division by a constant.
// No row fails.  A row whose date lies outside years -262143 .. 262142 is null in every field and every truncation, so is a Time
// value outside one day, and a truncation whose result does not fit the raw integer or -- the Monday of the first week -- lies
// before the range.  (unpinned-by-reference)
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CHQ_TEMPORAL_HD __host__ __device__
#else
#define CHQ_TEMPORAL_HD
#endif

namespace chq {

// the source kinds: one instantiation of the row rules each
enum TemporalKind : int32_t {
  TK_DATE32 = 0, TK_DATE64, TK_TS_S, TK_TS_MS, TK_TS_US, TK_TS_NS, TK_TIME32_S, TK_TIME32_MS, TK_TIME64_US, TK_TIME64_NS, TK_NKINDS
};
// EXTRACT / date_part fields (`week` is the ISO 8601 week, `dow` counts from Sunday = 0, `second` is whole seconds)
enum TemporalField : int32_t { TF_YEAR = 0, TF_QUARTER, TF_MONTH, TF_WEEK, TF_DAY, TF_DOY, TF_DOW, TF_HOUR, TF_MINUTE, TF_SECOND, TF_NFIELDS };
// date_trunc units (`week` starts on Monday)
enum TemporalUnit : int32_t { TU_YEAR = 0, TU_QUARTER, TU_MONTH, TU_WEEK, TU_DAY, TU_HOUR, TU_MINUTE, TU_SECOND, TU_NUNITS };

constexpr int TEMPORAL_GRID_CAP = 256 * 32;   // workgroups of a launch (typed_ops.h: rows_grid); the rows behind them are walked in rounds

CHQ_TEMPORAL_HD constexpr bool temporal_is_time(int kind) { return kind >= TK_TIME32_S; }
CHQ_TEMPORAL_HD constexpr bool temporal_is_i32(int kind) { return kind == TK_DATE32 || kind == TK_TIME32_S || kind == TK_TIME32_MS; }
// raw units per second (Date32: none, its raw value is the day number)
CHQ_TEMPORAL_HD constexpr int64_t temporal_units_per_second(int kind) {
  return kind == TK_TS_S || kind == TK_TIME32_S ? 1
         : kind == TK_DATE64 || kind == TK_TS_MS || kind == TK_TIME32_MS ? 1000
         : kind == TK_TS_US || kind == TK_TIME64_US ? 1000000
         : kind == TK_TS_NS || kind == TK_TIME64_NS ? 1000000000 : 0;
}

// ---- the calendar on 32-bit day numbers -----------------------------------------------------------------------------------------
// Day numbers and years are shifted by whole 400-year eras so that every dividend is non-negative: unsigned division by a
// constant, which compiles to a multiply and a shift.
constexpr int32_t kEraDays = 146097, kEraShift = 700;          // 700 eras = 280 000 years
constexpr int32_t kDaysToMarch0 = 719468;                      // 0000-03-01 is day -719468
constexpr int32_t kMinDay = -96465292, kMaxDay = 95026236;     // -262143-01-01 and 262142-12-31

struct CivilDate { int32_t year, month, day, doy_march; };     // doy_march: days since March 1st, [0, 365]

CHQ_TEMPORAL_HD inline bool temporal_is_leap(int32_t year) {
  const uint32_t y = (uint32_t)(year + 400 * kEraShift);
  return (y % 4u == 0 && y % 100u != 0) || y % 400u == 0;
}
CHQ_TEMPORAL_HD inline CivilDate civil_from_days(int32_t days) {
  const uint32_t z = (uint32_t)(days + kDaysToMarch0 + kEraDays * kEraShift);
  const uint32_t era = z / 146097u;
  const uint32_t doe = z - era * 146097u;                                        // [0, 146096]
  const uint32_t yoe = (doe - doe / 1460u + doe / 36524u - doe / 146096u) / 365u;   // [0, 399]
  const uint32_t doy = doe - (365u * yoe + yoe / 4u - yoe / 100u);               // [0, 365]
  const uint32_t mp = (5u * doy + 2u) / 153u;                                    // [0, 11], March = 0
  CivilDate c;
  c.day = (int32_t)(doy - (153u * mp + 2u) / 5u + 1u);
  c.month = (int32_t)(mp < 10u ? mp + 3u : mp - 9u);
  c.year = (int32_t)yoe + ((int32_t)era - kEraShift) * 400 + (c.month <= 2 ? 1 : 0);
  c.doy_march = (int32_t)doy;
  return c;
}
CHQ_TEMPORAL_HD inline int32_t days_from_civil(int32_t year, int32_t month, int32_t day) {
  const uint32_t y = (uint32_t)(year - (month <= 2 ? 1 : 0) + 400 * kEraShift);
  const uint32_t era = y / 400u;
  const uint32_t yoe = y - era * 400u;
  const uint32_t doy = (153u * (uint32_t)(month > 2 ? month - 3 : month + 9) + 2u) / 5u + (uint32_t)(day - 1);
  const uint32_t doe = yoe * 365u + yoe / 4u - yoe / 100u + doy;
  return ((int32_t)era - kEraShift) * kEraDays + (int32_t)doe - kDaysToMarch0;
}
// Sunday = 0 (1970-01-01 was a Thursday)
CHQ_TEMPORAL_HD inline int32_t day_of_week(int32_t days) { return (int32_t)((uint32_t)(days + 4 + 7 * 20000000) % 7u); }
// 1 .. 366
CHQ_TEMPORAL_HD inline int32_t day_of_year(const CivilDate& c) {
  return c.month > 2 ? c.doy_march + 60 + (temporal_is_leap(c.year) ? 1 : 0) : c.doy_march - 305;
}
// ISO 8601: weeks start on Monday, week 1 holds the year's first Thursday.  A date in the last week of the year before is
// numbered as a day of that year; one of week 53 that belongs to week 1 of the year after is week 1.
CHQ_TEMPORAL_HD inline int32_t iso_week(const CivilDate& c, int32_t days) {
  const int32_t wd = (day_of_week(days) + 6) % 7 + 1;   // Monday = 1 .. Sunday = 7
  const int32_t doy = day_of_year(c);
  const int32_t len = 365 + (temporal_is_leap(c.year) ? 1 : 0), len_before = 365 + (temporal_is_leap(c.year - 1) ? 1 : 0);
  int32_t n = doy - wd + 10;
  if (n < 7) n += len_before;
  else if (n - len >= 7) n -= len;
  return (int32_t)((uint32_t)n / 7u);
}

// ---- the floor split ---------------------------------------------------------------------------------------------------------
// raw = days * per_day + rem with 0 <= rem < per_day; `days` stays 64-bit until the range check
template <int64_t PER_DAY>
CHQ_TEMPORAL_HD inline void floor_split(int64_t raw, int64_t* days, int64_t* rem) {
  int64_t q = raw / PER_DAY, r = raw - q * PER_DAY;
  if (r < 0) { r += PER_DAY; q -= 1; }
  *days = q; *rem = r;
}

// ---- EXTRACT / date_part: false = the row is null --------------------------------------------------------------------------
template <int KIND>
CHQ_TEMPORAL_HD inline bool temporal_part_of(int field, int64_t raw, int32_t* out) {
  constexpr int64_t UPS = KIND == TK_DATE32 ? 1 : temporal_units_per_second(KIND);
  constexpr int64_t PER_DAY = 86400 * UPS;
  int64_t days64, rem;
  if (KIND == TK_DATE32) { days64 = raw; rem = 0; }
  else if (temporal_is_time(KIND)) { days64 = 0; rem = raw; if (raw < 0 || raw >= PER_DAY) return false; }
  else floor_split<PER_DAY>(raw, &days64, &rem);
  if (days64 < kMinDay || days64 > kMaxDay) return false;
  if (field >= TF_HOUR) {
    // whole seconds since midnight, [0, 86400): a 32-bit division where a day of units fits 32 bits (seconds, milliseconds), one
    // more 64-bit division by a constant where it does not (microseconds, nanoseconds); 32-bit from there on
    const uint32_t secs = PER_DAY <= (int64_t)UINT32_MAX ? (uint32_t)rem / (uint32_t)UPS : (uint32_t)((uint64_t)rem / (uint64_t)UPS);
    if (field == TF_HOUR) *out = (int32_t)(secs / 3600u);
    else if (field == TF_MINUTE) *out = (int32_t)(secs / 60u % 60u);
    else *out = (int32_t)(secs % 60u);
    return true;
  }
  const int32_t days = (int32_t)days64;
  if (field == TF_DOW) { *out = day_of_week(days); return true; }
  const CivilDate c = civil_from_days(days);
  switch (field) {
    case TF_YEAR: *out = c.year; break;
    case TF_QUARTER: *out = (int32_t)((uint32_t)(c.month + 2) / 3u); break;
    case TF_MONTH: *out = c.month; break;
    case TF_WEEK: *out = iso_week(c, days); break;
    case TF_DAY: *out = c.day; break;
    default: *out = day_of_year(c); break;
  }
  return true;
}

// ---- date_trunc: false = the row is null -----------------------------------------------------------------------------------
template <int KIND>
CHQ_TEMPORAL_HD inline bool temporal_trunc_of(int unit, int64_t raw, int64_t* out) {
  constexpr int64_t UPS = KIND == TK_DATE32 ? 1 : temporal_units_per_second(KIND);
  constexpr int64_t PER_DAY = KIND == TK_DATE32 ? 1 : 86400 * UPS;
  int64_t days64, rem;
  if (KIND == TK_DATE32) { days64 = raw; rem = 0; }
  else floor_split<PER_DAY>(raw, &days64, &rem);
  if (days64 < kMinDay || days64 > kMaxDay) return false;
  if (unit > TU_DAY) {   // inside the day: the value less what its time of day holds beyond the unit
    if (KIND == TK_DATE32) { *out = raw; return true; }
    // what the time of day holds beyond the unit: 32-bit where a day of units fits 32 bits, else one 64-bit remainder by a constant
    uint64_t cut;
    if (PER_DAY <= (int64_t)UINT32_MAX) {
      const uint32_t t = (uint32_t)rem;
      cut = unit == TU_HOUR ? t % (uint32_t)(3600 * UPS) : unit == TU_MINUTE ? t % (uint32_t)(60 * UPS) : t % (uint32_t)UPS;
    } else {
      const uint64_t t = (uint64_t)rem;
      cut = unit == TU_HOUR ? t % (uint64_t)(3600 * UPS) : unit == TU_MINUTE ? t % (uint64_t)(60 * UPS) : t % (uint64_t)UPS;
    }
    if (raw < INT64_MIN + (int64_t)cut) return false;
    *out = raw - (int64_t)cut;
    return true;
  }
  int32_t days = (int32_t)days64;
  if (unit == TU_WEEK) {
    days -= (day_of_week(days) + 6) % 7;
    if (days < kMinDay) return false;   // (the Monday of the range's first week lies before the range)
  } else if (unit != TU_DAY) {
    const CivilDate c = civil_from_days(days);
    const int32_t month = unit == TU_YEAR ? 1 : unit == TU_QUARTER ? (int32_t)((uint32_t)(c.month - 1) / 3u) * 3 + 1 : c.month;
    days = days_from_civil(c.year, month, 1);
  }
  // (C++ division truncates toward zero: the quotients are the least and the greatest day whose product fits)
  if (KIND != TK_DATE32 && (days < INT64_MIN / PER_DAY || days > INT64_MAX / PER_DAY)) return false;
  *out = (int64_t)days * PER_DAY;
  return true;
}

// the same with the kind read at run time: the host's entry (plan.cpp, the tests' program); the kernels instantiate the templates
CHQ_TEMPORAL_HD inline bool temporal_part(int kind, int field, int64_t raw, int32_t* out) {
  switch (kind) {
    case TK_DATE32: return temporal_part_of<TK_DATE32>(field, raw, out);
    case TK_DATE64: case TK_TS_MS: return temporal_part_of<TK_TS_MS>(field, raw, out);
    case TK_TS_S: return temporal_part_of<TK_TS_S>(field, raw, out);
    case TK_TS_US: return temporal_part_of<TK_TS_US>(field, raw, out);
    case TK_TS_NS: return temporal_part_of<TK_TS_NS>(field, raw, out);
    case TK_TIME32_S: return temporal_part_of<TK_TIME32_S>(field, raw, out);
    case TK_TIME32_MS: return temporal_part_of<TK_TIME32_MS>(field, raw, out);
    case TK_TIME64_US: return temporal_part_of<TK_TIME64_US>(field, raw, out);
    case TK_TIME64_NS: return temporal_part_of<TK_TIME64_NS>(field, raw, out);
    default: return false;
  }
}
CHQ_TEMPORAL_HD inline bool temporal_trunc(int kind, int unit, int64_t raw, int64_t* out) {
  switch (kind) {
    case TK_DATE32: return temporal_trunc_of<TK_DATE32>(unit, raw, out);
    case TK_DATE64: case TK_TS_MS: return temporal_trunc_of<TK_TS_MS>(unit, raw, out);
    case TK_TS_S: return temporal_trunc_of<TK_TS_S>(unit, raw, out);
    case TK_TS_US: return temporal_trunc_of<TK_TS_US>(unit, raw, out);
    case TK_TS_NS: return temporal_trunc_of<TK_TS_NS>(unit, raw, out);
    default: return false;
  }
}

// ---- DATE '..' / TIMESTAMP '..' ----------------------------------------------------------------------------------------------
// The spelling: YYYY-MM-DD, for a TIMESTAMP followed by ' ' or 'T' and HH:MM[:SS[.f{1,9}]]; years 0001 - 9999, a day the
// proleptic Gregorian calendar has, no zone suffix, no white space around it.
struct TemporalLiteral { int32_t days; int32_t second_of_day; int32_t nanos; int32_t fraction_digits; };
enum { TEMPORAL_LIT_DATE = 0, TEMPORAL_LIT_TIMESTAMP = 1 };

inline bool temporal_parse_literal(int lit_kind, const char* s, int64_t n, TemporalLiteral* out) {
  auto digits = [&](int64_t at, int count, int32_t* v) {
    if (at + count > n) return false;
    int32_t acc = 0;
    for (int k = 0; k < count; ++k) { const char c = s[at + k]; if (c < '0' || c > '9') return false; acc = acc * 10 + (c - '0'); }
    *v = acc;
    return true;
  };
  int32_t y, m, d, hh = 0, mi = 0, ss = 0, nanos = 0, fd = 0;
  if (n < 10 || !digits(0, 4, &y) || s[4] != '-' || !digits(5, 2, &m) || s[7] != '-' || !digits(8, 2, &d)) return false;
  if (y < 1 || m < 1 || m > 12 || d < 1) return false;
  static const int kLen[12] = {31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31};
  if (d > kLen[m - 1] + (m == 2 && temporal_is_leap(y) ? 1 : 0)) return false;
  if (lit_kind == TEMPORAL_LIT_DATE) {
    if (n != 10) return false;
  } else {
    if (n < 16 || (s[10] != ' ' && s[10] != 'T') || !digits(11, 2, &hh) || s[13] != ':' || !digits(14, 2, &mi)) return false;
    int64_t at = 16;
    if (at < n) {
      if (s[at] != ':' || !digits(at + 1, 2, &ss)) return false;
      at += 3;
      if (at < n) {
        if (s[at] != '.') return false;
        ++at;
        while (at < n && fd < 9 && s[at] >= '0' && s[at] <= '9') { nanos = nanos * 10 + (s[at] - '0'); ++at; ++fd; }
        if (fd == 0 || at != n) return false;
        for (int k = fd; k < 9; ++k) nanos *= 10;
      }
    }
    if (hh > 23 || mi > 59 || ss > 59) return false;
  }
  out->days = days_from_civil(y, m, d);
  out->second_of_day = hh * 3600 + mi * 60 + ss;
  out->nanos = nanos; out->fraction_digits = fd;
  return true;
}
// The literal as a raw value of a column of `kind` (not a Time kind).  0 = fine; 1 = it holds fraction digits finer than the
// unit (a truncated bound would move rows); 2 = the value does not fit the unit's integer.
inline int temporal_literal_raw(const TemporalLiteral& lit, int kind, int64_t* out) {
  if (kind == TK_DATE32) { *out = lit.days; return 0; }
  const int64_t ups = temporal_units_per_second(kind);
  const int64_t per_unit_ns = 1000000000 / ups;
  if (lit.nanos % per_unit_ns != 0) return 1;
  const __int128 v = ((__int128)lit.days * 86400 + lit.second_of_day) * ups + lit.nanos / per_unit_ns;
  if (v < (__int128)INT64_MIN || v > (__int128)INT64_MAX) return 2;
  *out = (int64_t)v;
  return 0;
}

// ---- temporal.hip -----------------------------------------------------------------------------------------------------------
// temporal_part_kernel writes an Int32 column, temporal_trunc_kernel one of the input's width; a null row is written as 0.
struct TemporalParams {
  const void* values;             // the raw values, Int32 or Int64 by `kind`, read from element values_offset (a sliced view)
  int64_t values_offset;
  const void* validity;           // or null: no nulls; read from bit validity_offset
  int64_t validity_offset;
  int64_t nrows;
  int32_t kind;                   // TemporalKind
  int32_t op;                     // TemporalField / TemporalUnit: wave-uniform
  void* out_values;
  unsigned long long* out_validity;   // (nrows + 63) / 64 words
  unsigned long long* null_count;
};

}  // namespace chq
