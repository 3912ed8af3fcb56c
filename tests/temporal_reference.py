"""The tests' reference for DATE / TIMESTAMP literals, EXTRACT / date_part and date_trunc, on Python
ints.  It is written from the calendar's definition -- a table of the year starts of one 400-year cycle, a table of month
lengths, `divmod` -- and shares nothing with csrc/temporal_device.h, which computes the same without tables.

A value is the raw integer of its Arrow column.  `part(kind, field, raw)` and `trunc(kind, unit, raw)` answer an int, or None
where the library's null rule makes the row null: a date outside years -262143 .. 262142, a Time value outside one day, a
truncated value that does not fit the raw integer or lies before the first day of the range."""
import bisect
import random
import re

import pyarrow as pa

FIELDS = ("year", "quarter", "month", "week", "day", "doy", "dow", "hour", "minute", "second")
UNITS = ("year", "quarter", "month", "week", "day", "hour", "minute", "second")
MIN_YEAR, MAX_YEAR = -262143, 262142


class Kind:
    def __init__(self, name, code, arrow, bits, per_second, is_time=False):
        self.name, self.code, self.arrow, self.bits, self.per_second, self.is_time = name, code, arrow, bits, per_second, is_time
        self.per_day = None if per_second is None else 86400 * per_second
        self.lo, self.hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1


# code = the TemporalKind number of csrc/temporal_device.h
KINDS = {k.name: k for k in (
    Kind("date32", 0, pa.date32(), 32, None), Kind("date64", 1, pa.date64(), 64, 1000),
    Kind("ts_s", 2, pa.timestamp("s"), 64, 1), Kind("ts_ms", 3, pa.timestamp("ms"), 64, 10**3),
    Kind("ts_us", 4, pa.timestamp("us"), 64, 10**6), Kind("ts_ns", 5, pa.timestamp("ns"), 64, 10**9),
    Kind("time32_s", 6, pa.time32("s"), 32, 1, True), Kind("time32_ms", 7, pa.time32("ms"), 32, 10**3, True),
    Kind("time64_us", 8, pa.time64("us"), 64, 10**6, True), Kind("time64_ns", 9, pa.time64("ns"), 64, 10**9, True))}
DATE_KINDS = tuple(k for k in KINDS if not KINDS[k].is_time)
TIME_KINDS = tuple(k for k in KINDS if KINDS[k].is_time)
TIME_FIELDS = ("hour", "minute", "second")


# ---- the calendar ---------------------------------------------------------------------------------------------------------------
def is_leap(y):
    return y % 4 == 0 and (y % 100 != 0 or y % 400 == 0)


MONTH_LEN = (31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31)
CYCLE_DAYS = 146097
# day, within a 400-year cycle that starts at a year divisible by 400, on which year k of the cycle starts
YEAR_START = [0]
for _y in range(400):
    YEAR_START.append(YEAR_START[-1] + (366 if is_leap(_y) else 365))
assert YEAR_START[400] == CYCLE_DAYS
EPOCH_IN_CYCLES = 719528          # days from 0000-01-01 to 1970-01-01
assert EPOCH_IN_CYCLES == 4 * CYCLE_DAYS + YEAR_START[370]      # 1970 = 4 * 400 + 370


def month_len(y, m):
    return 29 if m == 2 and is_leap(y) else MONTH_LEN[m - 1]


def days_from_civil(y, m, d):
    cycle, k = divmod(y, 400)
    return cycle * CYCLE_DAYS + YEAR_START[k] + sum(month_len(y, q) for q in range(1, m)) + (d - 1) - EPOCH_IN_CYCLES


def civil_from_days(days):
    """(year, month, day, day of year 1..366)"""
    cycle, n = divmod(days + EPOCH_IN_CYCLES, CYCLE_DAYS)
    k = bisect.bisect_right(YEAR_START, n) - 1
    y = cycle * 400 + k
    doy = n - YEAR_START[k]
    m, rest = 1, doy
    while rest >= month_len(y, m):
        rest -= month_len(y, m)
        m += 1
    return y, m, rest + 1, doy + 1


MIN_DAY, MAX_DAY = days_from_civil(MIN_YEAR, 1, 1), days_from_civil(MAX_YEAR, 12, 31)


def day_of_week(days):
    """Sunday = 0; 1970-01-01 was a Thursday"""
    return (days + 4) % 7


def iso_week(days):
    """ISO 8601: the week belongs to the year of its Thursday"""
    thursday = days - (days + 3) % 7 + 3          # (days + 3) % 7: Monday = 0
    y = civil_from_days(thursday)[0]
    return (thursday - days_from_civil(y, 1, 1)) // 7 + 1


# ---- the split and the null rule --------------------------------------------------------------------------------------------------
def split(kind, raw):
    """(days since 1970-01-01, units since midnight) by floor division, or None where the row is null"""
    K = KINDS[kind]
    if K.is_time:
        return (0, raw) if 0 <= raw < K.per_day else None
    days, rem = (raw, 0) if K.per_day is None else divmod(raw, K.per_day)
    return (days, rem) if MIN_DAY <= days <= MAX_DAY else None


def part(kind, field, raw):
    K = KINDS[kind]
    s = split(kind, raw)
    if s is None:
        return None
    days, rem = s
    if field in TIME_FIELDS:
        secs = 0 if K.per_second is None else rem // K.per_second
        return {"hour": secs // 3600, "minute": secs // 60 % 60, "second": secs % 60}[field]
    assert not K.is_time, (kind, field)
    if field == "dow":
        return day_of_week(days)
    if field == "week":
        return iso_week(days)
    y, m, d, doy = civil_from_days(days)
    return {"year": y, "quarter": (m - 1) // 3 + 1, "month": m, "day": d, "doy": doy}[field]


def trunc(kind, unit, raw):
    K = KINDS[kind]
    assert not K.is_time
    s = split(kind, raw)
    if s is None:
        return None
    days, rem = s
    per_day = 1 if K.per_day is None else K.per_day
    if unit in ("hour", "minute", "second"):
        if K.per_day is None:
            return raw
        step = {"hour": 3600, "minute": 60, "second": 1}[unit] * K.per_second
        out = days * per_day + rem // step * step
    else:
        if unit == "week":
            days -= (days + 3) % 7
            if days < MIN_DAY:      # the Monday of the range's first week lies before the range
                return None
        elif unit != "day":
            y, m, _, _ = civil_from_days(days)
            m = {"year": 1, "quarter": (m - 1) // 3 * 3 + 1, "month": m}[unit]
            days = days_from_civil(y, m, 1)
        out = days * per_day
    return out if K.lo <= out <= K.hi else None


def part_rows(kind, field, values, valid):
    """(values with 0 in the null slots, validity) of a column"""
    got = [part(kind, field, v) if ok else None for v, ok in zip(values, valid)]
    return [0 if g is None else g for g in got], [g is not None for g in got]


def trunc_rows(kind, unit, values, valid):
    got = [trunc(kind, unit, v) if ok else None for v, ok in zip(values, valid)]
    return [0 if g is None else g for g in got], [g is not None for g in got]


# ---- the literals ---------------------------------------------------------------------------------------------------------------
BAD, FINER, RANGE = "bad spelling", "finer than the unit", "does not fit"
_DATE = re.compile(r"(\d{4})-(\d{2})-(\d{2})\Z")
_TIMESTAMP = re.compile(r"(\d{4})-(\d{2})-(\d{2})[ T](\d{2}):(\d{2})(?::(\d{2})(?:\.(\d{1,9}))?)?\Z")


def parse_literal(is_timestamp, text):
    """(days, second of day, nanoseconds) or BAD"""
    if not text.isascii():
        return BAD
    m = (_TIMESTAMP if is_timestamp else _DATE).match(text)
    if not m:
        return BAD
    y, mo, d = int(m.group(1)), int(m.group(2)), int(m.group(3))
    if y < 1 or not 1 <= mo <= 12 or not 1 <= d <= month_len(y, mo):
        return BAD
    hh = mi = ss = nanos = 0
    if is_timestamp:
        hh, mi, ss = int(m.group(4)), int(m.group(5)), int(m.group(6) or 0)
        nanos = int((m.group(7) or "0").ljust(9, "0"))
        if hh > 23 or mi > 59 or ss > 59:
            return BAD
    return days_from_civil(y, mo, d), hh * 3600 + mi * 60 + ss, nanos


def literal_raw(is_timestamp, text, kind):
    """the raw value of the literal beside a column of `kind`, or BAD / FINER / RANGE"""
    p = parse_literal(is_timestamp, text)
    if p is BAD:
        return BAD
    days, secs, nanos = p
    K = KINDS[kind]
    if K.per_day is None:
        return days
    if nanos % (10**9 // K.per_second):
        return FINER
    v = (days * 86400 + secs) * K.per_second + nanos // (10**9 // K.per_second)
    return v if K.lo <= v <= K.hi else RANGE


# ---- edge tables ------------------------------------------------------------------------------------------------------------------
EDGE_DATES = [(2000, 2, 29), (1900, 2, 28), (1900, 3, 1), (2100, 2, 28), (2100, 3, 1), (2024, 2, 29), (2023, 12, 31), (2024, 1, 1),
              (2018, 12, 31), (2020, 12, 31), (2021, 1, 3), (2021, 1, 4), (2026, 12, 31), (1, 1, 1), (9999, 12, 31)]
ERA_EDGE = -719468          # 0000-03-01: where a 400-year era of the March-based calendar arithmetic begins
assert civil_from_days(ERA_EDGE)[:3] == (0, 3, 1) and civil_from_days(ERA_EDGE - 1)[:3] == (0, 2, 29)
EDGE_DAYS = [0, 1, -1] + [days_from_civil(*d) for d in EDGE_DATES] + \
            [ERA_EDGE - 1, ERA_EDGE, ERA_EDGE - CYCLE_DAYS, ERA_EDGE + CYCLE_DAYS,
             MIN_DAY - 1, MIN_DAY, MIN_DAY + 1, MAX_DAY - 1, MAX_DAY, MAX_DAY + 1]


def edges(kind):
    """the fixed edge table of a source type: raw values, in a fixed order, without repeats"""
    K = KINDS[kind]
    out = [0, 1, -1]
    if K.is_time:
        u = K.per_second
        out += [K.per_day - 1, K.per_day, K.per_day + 1, 3600 * u - 1, 3600 * u, 60 * u - 1, 60 * u, u - 1, u, 2 * u - 1,
                (13 * 3600 + 45 * 60 + 56) * u, (23 * 3600 + 59 * 60 + 59) * u, 12 * 3600 * u]
    elif K.per_day is None:
        out += EDGE_DAYS
    else:
        mid = (13 * 3600 + 45 * 60 + 56) * K.per_second + (K.per_second * 789 // 1000)
        for d in (1, -1):     # one unit either side of a day boundary, in both signs
            out += [d * K.per_day - 1, d * K.per_day, d * K.per_day + 1]
        for d in EDGE_DAYS:
            out += [d * K.per_day, d * K.per_day + K.per_day - 1, d * K.per_day + mid]
    out += [K.lo, K.lo + 1, K.hi - 1, K.hi]
    seen, table = set(), []
    for v in out:
        if K.lo <= v <= K.hi and v not in seen:
            seen.add(v)
            table.append(v)
    return table


def in_common_era(kind, raw):
    """the row is a date of years 1 .. 9999: what pyarrow and `datetime` can be asked about"""
    s = split(kind, raw)
    return s is not None and (KINDS[kind].is_time or days_from_civil(1, 1, 1) <= s[0] <= days_from_civil(9999, 12, 31))


def random_values(kind, n, seed=20240301):
    """n raw values from a fixed seed: a third over the whole raw type, a third within years 1 .. 9999, a third near the epoch"""
    K = KINDS[kind]
    rng = random.Random(seed + K.code)
    per_day = K.per_day or 1
    if K.is_time:
        return [rng.randrange(K.lo, K.hi + 1) if i % 3 == 0 else rng.randrange(0, per_day) for i in range(n)]
    lo_ce, hi_ce = max(K.lo, days_from_civil(1, 1, 1) * per_day), min(K.hi, days_from_civil(9999, 12, 31) * per_day + per_day - 1)
    lo_ep, hi_ep = max(K.lo, -40000 * per_day), min(K.hi, 40000 * per_day)
    return [rng.randrange(K.lo, K.hi + 1) if i % 3 == 0 else rng.randrange(lo_ce, hi_ce + 1) if i % 3 == 1 else rng.randrange(lo_ep, hi_ep + 1)
            for i in range(n)]
