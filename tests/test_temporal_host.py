"""CPU: DATE / TIMESTAMP literals, EXTRACT / date_part and date_trunc without a GPU.  The tests' reference
(tests/temporal_reference.py) against pyarrow.compute and `datetime` on the rows they can be asked about, and against calendar
identities on the rest and on random values; the grammar; the library's host half (typing, status codes, the literal conversion,
the lowered program) through `chq_plan_describe`; the per-row code of csrc/temporal_device.h alone in a stand-alone program under
the address and undefined-behaviour sanitizers; and the row count tests/test_gpu_temporal.py uses to reach the second round of
the capped grid, held to the sources."""
import datetime
import os
import re
import shutil
import subprocess

import pyarrow as pa
import pyarrow.compute as pc
import pytest

import chapterhouseqe_amd as chq
from chapterhouseqe_amd import sqlast as A
from chapterhouseqe_amd.sqlparse import SqlParseError, parse_expr, parse_select

from . import temporal_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "chapterhouseqe_amd", "csrc")
NOT_SUPPORTED, CAST_ERROR, INVALID_ARGUMENT, COERSION, NOT_IMPLEMENTED = 30, 24, 22, 9, 2
N_RANDOM = 100_000
EPOCH_ORDINAL = datetime.date(1970, 1, 1).toordinal()


# ---- the reference against pyarrow and datetime ------------------------------------------------------------------------------------
PC_FIELD = {"year": pc.year, "quarter": pc.quarter, "month": pc.month, "week": pc.iso_week, "day": pc.day, "doy": pc.day_of_year,
            "dow": lambda a: pc.day_of_week(a, count_from_zero=True, week_start=7), "hour": pc.hour, "minute": pc.minute, "second": pc.second}


def arrow_twin(kind):
    """the type pyarrow is asked with: Date64 through the same raw values as Timestamp(ms) (pyarrow has no `hour` for it)"""
    return pa.timestamp("ms") if kind == "date64" else R.KINDS[kind].arrow


@pytest.mark.parametrize("kind", list(R.KINDS))
def test_reference_agrees_with_pyarrow_on_the_edge_table(kind):
    table = R.edges(kind)
    vals = [v for v in table if R.in_common_era(kind, v)]
    assert 2 * len(vals) >= len(table), (kind, len(vals), len(table))       # at least half of the table is pinned to pyarrow
    arr = pa.array(vals, pa.int32() if R.KINDS[kind].bits == 32 else pa.int64()).cast(arrow_twin(kind))
    fields = R.TIME_FIELDS if R.KINDS[kind].is_time else [f for f in R.FIELDS if kind != "date32" or f not in R.TIME_FIELDS]
    for field in fields:
        assert PC_FIELD[field](arr).to_pylist() == [R.part(kind, field, v) for v in vals], (kind, field)
    if kind == "date32":
        assert all(R.part(kind, f, v) == 0 for f in R.TIME_FIELDS for v in vals)
    if not R.KINDS[kind].is_time:
        for unit in R.UNITS:
            got = pc.floor_temporal(arr, unit=unit, week_starts_monday=True).cast(pa.int32() if kind == "date32" else pa.int64()).to_pylist()
            want = [R.trunc(kind, unit, v) for v in vals]
            # (where the floor lies below Int64 -- the first days of Timestamp(ns) -- pyarrow wraps around; the rule here is null)
            assert all(w is not None or (kind == "ts_ns" and v < 0) for w, v in zip(want, vals)), (kind, unit)
            # (.. and so it does in its week arithmetic within days of either end of Int64: the test against `datetime` pins those rows)
            near_end = lambda v: kind == "ts_ns" and min(v - R.KINDS[kind].lo, R.KINDS[kind].hi - v) < 8 * R.KINDS[kind].per_day
            assert [(v, g, w) for v, g, w in zip(vals, got, want) if w is not None and g != w and not near_end(v)] == [], (kind, unit)


@pytest.mark.parametrize("kind", R.DATE_KINDS)
def test_reference_agrees_with_datetime_on_the_edge_table(kind):
    vals = [v for v in R.edges(kind) if R.in_common_era(kind, v)]
    for v in vals:
        days, rem = R.split(kind, v)
        d = datetime.date.fromordinal(days + EPOCH_ORDINAL)
        assert (R.part(kind, "year", v), R.part(kind, "month", v), R.part(kind, "day", v)) == (d.year, d.month, d.day), (kind, v)
        assert R.part(kind, "week", v) == d.isocalendar()[1] and R.part(kind, "dow", v) == (d.weekday() + 1) % 7, (kind, v)
        assert R.part(kind, "doy", v) == d.timetuple().tm_yday and R.days_from_civil(d.year, d.month, d.day) == d.toordinal() - EPOCH_ORDINAL
        monday = d - datetime.timedelta(days=d.weekday())
        per_day = R.KINDS[kind].per_day or 1
        if monday.year >= 1 and not (kind == "ts_ns" and monday.toordinal() - EPOCH_ORDINAL < -106751):      # (a Monday before Int64 nanoseconds begin: null)
            assert R.trunc(kind, "week", v) == (monday.toordinal() - EPOCH_ORDINAL) * per_day, (kind, v)


def test_edge_tables_hold_what_they_must():
    days = {R.days_from_civil(*d) for d in R.EDGE_DATES} | {0, 1, -1, R.ERA_EDGE, R.ERA_EDGE - 1, R.ERA_EDGE - R.CYCLE_DAYS, R.ERA_EDGE + R.CYCLE_DAYS,
                                                           R.MIN_DAY - 1, R.MIN_DAY, R.MIN_DAY + 1, R.MAX_DAY - 1, R.MAX_DAY, R.MAX_DAY + 1}
    assert days <= set(R.edges("date32")) and {R.KINDS["date32"].lo, R.KINDS["date32"].hi} <= set(R.edges("date32"))
    for kind in ("date64", "ts_s", "ts_ms", "ts_us", "ts_ns"):
        K, table = R.KINDS[kind], set(R.edges(kind))
        assert {0, 1, -1, K.lo, K.hi, K.per_day - 1, K.per_day, K.per_day + 1, -K.per_day - 1, -K.per_day, -K.per_day + 1} <= table
        assert {d * K.per_day for d in days if K.lo <= d * K.per_day <= K.hi} <= table
    assert len([d for d in days if R.KINDS["ts_s"].lo <= d * 86400 <= R.KINDS["ts_s"].hi]) == len(days)      # seconds reach every date
    assert R.civil_from_days(R.MIN_DAY)[:3] == (-262143, 1, 1) and R.civil_from_days(R.MAX_DAY)[:3] == (262142, 12, 31)


# ---- identities, where nothing else can be asked -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.DATE_KINDS)
def test_identities_on_the_edge_table_and_on_random_values(kind):
    K = R.KINDS[kind]
    values = R.edges(kind) + R.random_values(kind, N_RANDOM)
    above = {"year": ("year",), "quarter": ("year", "quarter"), "month": ("year", "quarter", "month"), "week": (),
             "day": ("year", "month", "day"), "hour": ("year", "doy", "hour"), "minute": ("doy", "hour", "minute"), "second": ("hour", "minute", "second")}
    for i, v in enumerate(values):
        s = R.split(kind, v)
        days = v if K.per_day is None else v // K.per_day
        assert (s is None) == (not R.MIN_DAY <= days <= R.MAX_DAY)               # the null rule, exactly
        if s is None:
            assert all(R.part(kind, f, v) is None for f in ("year", "dow", "hour")) and R.trunc(kind, "day", v) is None
            continue
        y, m, d, doy = R.civil_from_days(s[0])
        assert R.days_from_civil(y, m, d) == s[0] and R.days_from_civil(y, 1, 1) + doy - 1 == s[0]
        # (the edge table takes every unit, a random value one of them in turn)
        for unit in (R.UNITS if i < len(values) - N_RANDOM else (R.UNITS[i % len(R.UNITS)],)):
            t = R.trunc(kind, unit, v)
            if t is None:      # only where the truncated value does not fit the raw integer, or is a Monday before the range
                assert (kind == "ts_ns" and v < K.lo + 366 * K.per_day) or (unit == "week" and days < R.MIN_DAY + 7), (kind, unit, v)
                continue
            assert t <= v and R.trunc(kind, unit, t) == t, (kind, unit, v)
            if R.split(kind, t) is not None:
                assert all(R.part(kind, f, t) == R.part(kind, f, v) for f in above[unit]), (kind, unit, v)
            if unit == "week" and R.split(kind, t) is not None:
                assert R.part(kind, "dow", t) == 1 and 0 <= (v - t) // (K.per_day or 1) < 7
    for edge, inside in ((R.MIN_DAY, True), (R.MIN_DAY - 1, False), (R.MAX_DAY, True), (R.MAX_DAY + 1, False)):
        raw = edge if K.per_day is None else edge * K.per_day
        if K.lo <= raw <= K.hi:
            assert (R.part(kind, "year", raw) is not None) == inside and (R.part(kind, "hour", raw) is not None) == inside, (kind, edge)
    assert R.part(kind, "year", K.lo) is None or kind == "ts_ns"
    if kind == "ts_ns":      # the most negative values: a date in 1677, whose day -- and hour -- floor lies below Int64
        assert R.part(kind, "year", K.lo) == 1677 and R.trunc(kind, "day", K.lo) is None and R.trunc(kind, "hour", K.lo) is None
        assert R.trunc(kind, "second", K.lo) is None and R.trunc(kind, "second", K.lo + 10**9) is not None
    if kind == "ts_s":
        assert (R.part(kind, "year", -1), R.part(kind, "doy", -1), R.part(kind, "hour", -1), R.part(kind, "second", -1)) == (1969, 365, 23, 59)


@pytest.mark.parametrize("kind", R.TIME_KINDS)
def test_time_values_outside_one_day_are_null(kind):
    K = R.KINDS[kind]
    for v in R.edges(kind) + R.random_values(kind, N_RANDOM):
        inside = 0 <= v < K.per_day
        for f in R.TIME_FIELDS:
            assert (R.part(kind, f, v) is not None) == inside
        if inside:
            secs = v // K.per_second
            assert R.part(kind, "hour", v) * 3600 + R.part(kind, "minute", v) * 60 + R.part(kind, "second", v) == secs


# ---- grammar ---------------------------------------------------------------------------------------------------------------------------
B, Op = A.BinaryOp, A.BinaryOperator
DATE, TIMESTAMP = A.TypedStringType.Date, A.TypedStringType.Timestamp


def test_grammar_typed_strings():
    assert parse_expr("DATE '2024-03-01'") == A.TypedString(DATE, "2024-03-01") == parse_expr("date '2024-03-01'")
    assert parse_expr("ts >= TIMESTAMP '2024-03-01 00:00:00'") == B(A.ident("ts"), Op.GtEq, A.TypedString(TIMESTAMP, "2024-03-01 00:00:00"))
    assert parse_expr("timestamp 'x' < ts") == B(A.TypedString(TIMESTAMP, "x"), Op.Lt, A.ident("ts"))         # the spelling is typing's business
    assert parse_expr("d between date '2024-01-01' and date '2024-12-31'") == \
        A.Between(A.ident("d"), False, A.TypedString(DATE, "2024-01-01"), A.TypedString(DATE, "2024-12-31"))
    assert parse_expr("d in (date '2024-01-01', date '2024-01-02')") == A.InList(A.ident("d"), (A.TypedString(DATE, "2024-01-01"), A.TypedString(DATE, "2024-01-02")))
    # `date` and `timestamp` stay ordinary words wherever no string literal follows
    assert parse_expr("date >= 5") == B(A.ident("date"), Op.GtEq, A.number("5")) and parse_expr("timestamp + 1") == B(A.ident("timestamp"), Op.Plus, A.number("1"))
    assert parse_expr("t.date = t.timestamp") == B(A.compound("t", "date"), Op.Eq, A.compound("t", "timestamp"))
    assert parse_expr("date = '2024-01-01'") == B(A.ident("date"), Op.Eq, A.string("2024-01-01"))
    assert isinstance(parse_expr("date(a)"), A.Function) and parse_expr("date(a)").name == "date"
    sel = parse_select("select date, timestamp ts, a date from read_files('x') where date > 1")
    assert sel.projection[0] == A.UnnamedExpr(A.ident("date")) and sel.projection[1] == A.ExprWithAlias(A.ident("timestamp"), A.Ident("ts"))
    assert sel.projection[2] == A.ExprWithAlias(A.ident("a"), A.Ident("date")) and sel.selection == B(A.ident("date"), Op.Gt, A.number("1"))
    assert int(DATE) == 0 and int(TIMESTAMP) == 1
    header = open(os.path.join(ROOT, "include", "chq.h")).read()
    assert "typedef enum chq_typed_string_kind { CHQ_TYPED_STRING_DATE = 0, CHQ_TYPED_STRING_TIMESTAMP = 1 } chq_typed_string_kind;" in header


def test_grammar_extract_and_the_calls():
    assert parse_expr("extract(year from ts)") == A.Extract("year", A.ident("ts")) == parse_expr("EXTRACT ( year FROM ts )")
    assert parse_expr("extract(YEAR from ts)") == A.Extract("YEAR", A.ident("ts")) and parse_expr("extract('dow' from ts)") == A.Extract("dow", A.ident("ts"))
    assert parse_expr("extract(month from a) < 7") == B(A.Extract("month", A.ident("a")), Op.Lt, A.number("7"))
    inner = parse_expr("extract(hour from date_trunc('day', ts))")
    assert isinstance(inner, A.Extract) and isinstance(inner.expr, A.Function) and inner.expr.name == "date_trunc"
    assert inner.expr.args == (A.string("day"), A.ident("ts")) and A.Extract("year", A.ident("ts")).args is None
    f = parse_expr("Date_Part('year', ts)")
    assert isinstance(f, A.Function) and f.name == "Date_Part" and f.args == (A.string("year"), A.ident("ts"))
    assert parse_expr("extract + 1") == B(A.ident("extract"), Op.Plus, A.number("1"))            # a column called extract
    assert isinstance(parse_expr("extract(a, b)"), A.Function)                                     # no FROM: a call like before
    sel = parse_select("select date_trunc('month', ts) m, extract(doy from d) n from read_files('x') where extract(dow from ts) in (0, 6)")
    assert sel.projection[1] == A.ExprWithAlias(A.Extract("doy", A.ident("d")), A.Ident("n"))
    assert sel.selection == A.InList(A.Extract("dow", A.ident("ts")), (A.number("0"), A.number("6")))
    with pytest.raises(SqlParseError):
        parse_expr("extract(year from)")
    # HAVING: an aggregate under EXTRACT is rewritten to its hidden column, as under CAST
    from chapterhouseqe_amd.sqlparse import having_plan
    pred = having_plan(parse_select("select k, count(*) n from read_files('x') group by k having extract(year from max(ts)) = 2024"))[2]
    assert pred == B(A.Extract("year", A.ident("__having_0")), Op.Eq, A.number("2024"))


# ---- the library's host half -----------------------------------------------------------------------------------------------------------
SCHEMA = pa.schema([("d", pa.date32()), ("d64", pa.date64()), ("ts_s", pa.timestamp("s")), ("ts_ms", pa.timestamp("ms")), ("ts_us", pa.timestamp("us")),
                    ("ts_ns", pa.timestamp("ns")), ("utc", pa.timestamp("us", "UTC")), ("zero", pa.timestamp("ms", "+00:00")),
                    ("paris", pa.timestamp("us", "Europe/Paris")), ("plus1", pa.timestamp("s", "+01:00")), ("t32", pa.time32("s")), ("t32m", pa.time32("ms")),
                    ("t64", pa.time64("us")), ("t64n", pa.time64("ns")), ("dur", pa.duration("s")), ("dec", pa.decimal128(30, 2)), ("id", pa.int32()),
                    ("big", pa.int64()), ("f", pa.float32()), ("s", pa.utf8()), ("b", pa.bool_()), ("d2", pa.date32()), ("ts_us2", pa.timestamp("us"))])
COLUMN = {"date32": "d", "date64": "d64", "ts_s": "ts_s", "ts_ms": "ts_ms", "ts_us": "ts_us", "ts_ns": "ts_ns", "time32_s": "t32", "time32_ms": "t32m",
          "time64_us": "t64", "time64_ns": "t64n"}


def describe(expr, rows=2):
    try:
        return 0, chq.plan_describe(SCHEMA, None, parse_expr(expr) if isinstance(expr, str) else expr, rows)
    except chq.ChqError as e:
        return e.code, str(e)


def program(expr):
    code, out = describe(expr)
    assert code == 0 and "\nprogram " in out, (expr, out)
    return [re.sub(r"idx=\d+", "idx=_", ln) for ln in out.splitlines() if ln.startswith("  ")], out.splitlines()[0]


def const_of(expr):
    """the immediate of the one constant instruction"""
    lines, _ = program(expr)
    imms = [int(ln.rsplit("imm=0x", 1)[1], 16) for ln in lines if " const " in ln]
    assert len(imms) == 1, lines
    return imms[0]


def test_literal_lowers_to_the_integer_compare():
    want = R.literal_raw(True, "2024-03-01 00:00:00", "ts_us")
    assert want == 1709251200 * 10**6
    assert program("ts_us >= TIMESTAMP '2024-03-01 00:00:00'") == program(f"big >= {want}")          # the same program, FAST_CMP_CONST included
    assert program("TIMESTAMP '2024-03-01 00:00:00' <= ts_us") == program(f"{want} <= big")
    assert program("d < DATE '2024-03-01'") == program(f"id < {R.literal_raw(False, '2024-03-01', 'date32')}")
    assert program("utc >= TIMESTAMP '2024-03-01T00:00'")[0] == program(f"big >= {want}")[0]
    for sql, ops in (("d between DATE '2024-01-01' and DATE '2024-12-31'", ["GE", "SPILL", "LOAD", "LE", "AND"]),
                     ("d not between DATE '2024-01-01' and DATE '2024-12-31'", ["LT", "SPILL", "LOAD", "GT", "OR"]),
                     ("ts_s in (TIMESTAMP '2024-01-01 00:00', TIMESTAMP '2024-01-02 00:00')", ["EQ", "SPILL", "LOAD", "EQ", "OR"])):
        assert [ln.split()[0] for ln in program(sql)[0]][1:] == ops, sql
    code, out = describe("d in (DATE '2024-01-01', 5)")
    assert code == COERSION, out


@pytest.mark.parametrize("kind", R.DATE_KINDS)
def test_unit_adoption_per_column_type(kind):
    col = COLUMN[kind]
    for text in ("2024-03-01", "1969-12-31", "0001-01-01", "9999-12-31", "2000-02-29"):
        want = R.literal_raw(False, text, kind)
        if want is R.RANGE:
            assert kind == "ts_ns" and describe(f"{col} = DATE '{text}'")[0] == CAST_ERROR
            continue
        assert const_of(f"{col} = DATE '{text}'") == want % 2**64 == const_of(f"DATE '{text}' = {col}"), (kind, text)
    if kind in ("date32", "date64"):
        code, out = describe(f"{col} >= TIMESTAMP '2024-03-01 00:00:00'")
        assert code == NOT_SUPPORTED and "TIMESTAMP" in out
        return
    digits = {"ts_s": 0, "ts_ms": 3, "ts_us": 6, "ts_ns": 9}[kind]
    for text in ("2024-03-01 12:34:56", "2024-03-01T12:34", "1969-12-31 23:59:59", "1970-01-01 00:00:00.5", "2024-03-01 00:00:00.123456789", "2024-03-01 00:00:00.120"):
        want = R.literal_raw(True, text, kind)
        code, out = describe(f"{col} < TIMESTAMP '{text}'")
        if want is R.FINER:      # the fraction rule: a truncated bound would move rows
            frac = text.split(".")[1].rstrip("0")
            assert len(frac) > digits and code == CAST_ERROR and text in out, (kind, text, out)
        else:
            assert code == 0 and const_of(f"{col} < TIMESTAMP '{text}'") == want % 2**64, (kind, text, out)
    # the range rule: Int64 nanoseconds end in 2262 and begin in 1677; every coarser unit holds years 1 .. 9999
    for text in ("2300-01-01 00:00:00", "1600-01-01 00:00:00", "2262-04-11 23:47:16.854775808", "1677-09-21 00:12:43.145224191"):
        code, out = describe(f"{col} < TIMESTAMP '{text}'")
        want = R.literal_raw(True, text, kind)
        assert (code == CAST_ERROR and text in out) if want in (R.RANGE, R.FINER) else code == 0, (kind, text, out)
        assert (want is R.RANGE) == (kind == "ts_ns") or want is R.FINER
    assert const_of("ts_ns <= TIMESTAMP '2262-04-11 23:47:16.854775807'") == 2**63 - 1
    assert const_of("ts_ns >= TIMESTAMP '1677-09-21 00:12:43.145224192'") == 2**63


def test_zones():
    want = R.literal_raw(True, "2024-03-01 00:00:00", "ts_us")
    assert const_of("utc >= TIMESTAMP '2024-03-01 00:00:00'") == want and const_of("DATE '2024-03-01' <= utc") == want
    assert const_of("zero = DATE '2024-03-01'") == want // 1000
    for col in ("paris", "plus1"):
        for sql in (f"{col} >= TIMESTAMP '2024-03-01 00:00:00'", f"DATE '2024-03-01' < {col}", f"extract(hour from {col})", f"date_trunc('day', {col})",
                    f"date_part('year', {col}) = 2024"):
            code, out = describe(sql)
            assert code == NOT_SUPPORTED and "zone" in out, (sql, out)
    assert describe("utc = utc")[0] == 0 and describe("extract(hour from utc)")[0] == 0 == describe("date_trunc('hour', zero)")[0]
    assert describe("utc = ts_us")[0] == COERSION      # two DataTypes, as before


def test_refusals_of_the_literal():
    for col in ("id", "big", "f", "s", "b"):      # every non-temporal neighbour: what `d < 5` answers
        for sql in (f"{col} < DATE '2024-01-01'", f"TIMESTAMP '2024-01-01 00:00' >= {col}", f"{col} between DATE '2024-01-01' and DATE '2024-01-02'"):
            assert describe(sql)[0] == COERSION == describe("d < 5")[0], sql
    assert describe("5 < DATE '2024-01-01'")[0] == COERSION == describe("DATE '2024-01-01' = 'x'")[0]
    for sql in ("DATE '2024-01-01'", "TIMESTAMP '2024-01-01 00:00'", "DATE '2024-01-01' < DATE '2024-01-02'", "DATE '2024-01-01' + 1", "d - DATE '2024-01-01'",
                "d + DATE '2024-01-01' > d", "DATE '2024-01-01' and b", "extract(year from DATE '2024-01-01')", "date_trunc('day', TIMESTAMP '2024-01-01 00:00')",
                "coalesce(d, DATE '2024-01-01')", "case when b then d else DATE '2024-01-01' end", "DATE '2024-01-01' is null", "length(DATE '2024-01-01')",
                "t32 < DATE '2024-01-01'", "t64 = TIMESTAMP '2024-01-01 00:00'", "dur < DATE '2024-01-01'", "dec = DATE '2024-01-01'",
                "DATE '2024-01-01' || 'x'", "(DATE '2024-01-01')"):
        code, out = describe(sql)
        assert code == NOT_SUPPORTED, (sql, code, out)
    assert describe("(d) < (DATE '2024-01-01')")[0] == 0
    # CAST keeps refusing temporal operands, and `cast(a as date)` is no type the grammar knows
    assert describe(A.Cast(A.ident("d"), A.CastType.Int32))[0] == NOT_SUPPORTED
    with pytest.raises(SqlParseError):
        parse_expr("cast(s as date)")


GOOD = [("2024-03-01", False), ("0001-01-01", False), ("9999-12-31", False), ("2000-02-29", False), ("1900-02-28", False), ("2400-02-29", False),
        ("2024-03-01 00:00", True), ("2024-03-01T23:59", True), ("2024-03-01 12:34:56", True), ("2024-03-01T12:34:56.7", True),
        ("1969-12-31 23:59:59.999999999", True), ("0001-01-01 00:00:00", True), ("9999-12-31 23:59:59.999", True), ("2024-12-31 23:59:59.000000001", True)]
BAD = [("", False), ("2024-3-01", False), ("2024-03-1", False), ("24-03-01", False), ("2023-02-29", False), ("1900-02-29", False), ("2100-02-29", False),
       ("2024-00-10", False), ("2024-13-01", False), ("2024-04-31", False), ("2024-01-00", False), ("0000-01-01", False), ("10000-01-01", False),
       (" 2024-03-01", False), ("2024-03-01 ", False), ("2024-03-01 00:00:00", False), ("2024/03/01", False), ("+024-03-01", False), ("2024-03-0١", False),
       ("2024-03-01", True), ("2024-03-01 ", True), ("2024-03-01 24:00:00", True), ("2024-03-01 12:60", True), ("2024-03-01 12:00:60", True),
       ("2024-03-01 12", True), ("2024-03-01 12:0", True), ("2024-03-01 1:00:00", True), ("2024-03-01 12:00:", True), ("2024-03-01 12:00:00.", True),
       ("2024-03-01 12:00:00.1234567890", True), ("2024-03-01 12:00:00Z", True), ("2024-03-01 12:00:00+00:00", True), ("2024-03-01 12:00:00 UTC", True),
       ("2024-03-01  12:00", True), ("2024-03-01t12:00", True), ("2024-03-01 12:00:00.5 ", True), ("2023-02-29 00:00", True), ("2024-03-01 -1:00", True),
       ("2024-03-01 12:00.5", True)]


def test_literal_parser_tables():
    for text, is_ts in GOOD:
        p = R.parse_literal(is_ts, text)
        assert p is not R.BAD, text
        dt = datetime.datetime.fromisoformat(text[:19] if is_ts else text)      # (datetime reads the seconds; the fraction is checked below)
        assert p[0] == dt.date().toordinal() - EPOCH_ORDINAL and p[1] == dt.hour * 3600 + dt.minute * 60 + dt.second, text
        for kind in R.DATE_KINDS:
            if is_ts and kind in ("date32", "date64"):
                continue
            col, want = COLUMN[kind], R.literal_raw(is_ts, text, kind)
            code, out = describe(f"{col} = {'TIMESTAMP' if is_ts else 'DATE'} '{text}'")
            if want in (R.FINER, R.RANGE):
                assert code == CAST_ERROR and text in out, (text, kind, out)
            else:
                assert code == 0 and const_of(f"{col} = {'TIMESTAMP' if is_ts else 'DATE'} '{text}'") == want % 2**64, (text, kind, out)
    assert R.literal_raw(True, "1969-12-31 23:59:59.999999999", "ts_ns") == -1 and R.literal_raw(True, "2024-03-01T12:34:56.7", "ts_ms") % 1000 == 700
    for text, is_ts in BAD:
        assert R.parse_literal(is_ts, text) is R.BAD, text
        code, out = describe(A.BinaryOp(A.ident("ts_us"), Op.Lt, A.TypedString(TIMESTAMP if is_ts else DATE, text)))
        assert code == CAST_ERROR and f"'{text}'" in out, (text, is_ts, code, out)
        # the spelling is judged where the literal stands, whatever stands beside it
        assert describe(A.BinaryOp(A.ident("id"), Op.Lt, A.TypedString(TIMESTAMP if is_ts else DATE, text)))[0] == CAST_ERROR


def temporal_lines(expr):
    code, out = describe(expr)
    assert code == 0, (expr, out)
    lines = out.splitlines()
    assert lines[1] == "split a temporal function runs as its own kernel", (expr, out)
    return lines[0], [ln[len("temporal "):] for ln in lines[2:] if ln.startswith("temporal ")]


def test_functions_type_as_the_rules_say():
    for kind, K in R.KINDS.items():
        col = COLUMN[kind]
        for field in R.FIELDS:
            for sql in (f"extract({field} from {col})", f"date_part('{field.upper()}', {col})", f"DATE_PART('{field}', ({col}))"):
                code, out = describe(sql)
                if K.is_time and field not in R.TIME_FIELDS:
                    assert code == INVALID_ARGUMENT and field in out, (sql, out)
                else:
                    assert temporal_lines(sql) == ("result Int32 scalar=0 len1=0", [f"part {field} kind={K.code}"]), sql
        for unit in R.UNITS:
            sql = f"date_trunc('{unit}', {col})"
            if K.is_time:
                code, out = describe(sql)
                assert code == INVALID_ARGUMENT and SCHEMA.field(col).type.equals(K.arrow) and "tt" in out, (sql, out)
            else:      # the result format: the operand's own, unit and zone included
                fmt = {"date32": "tdD", "date64": "tdm"}.get(kind, f"ts{kind[3]}:")
                assert temporal_lines(sql) == ("result FixedWidth scalar=0 len1=0", [f"trunc {unit} kind={K.code} format={fmt}"]), sql
    assert temporal_lines("date_trunc('day', utc)")[1] == ["trunc day kind=4 format=tsu:UTC"] and temporal_lines("Date_Trunc('WEEK', zero)")[1] == ["trunc week kind=3 format=tsm:+00:00"]
    # any other operand type: named; a field that is no string literal, or unknown: not supported
    for col, name in (("id", "Int32"), ("s", "Utf8"), ("f", "Float32"), ("b", "Boolean"), ("dur", "tDs"), ("dec", "d:30,2")):
        for sql in (f"extract(year from {col})", f"date_trunc('day', {col})"):
            code, out = describe(sql)
            assert code == INVALID_ARGUMENT and name in out, (sql, out)
    for sql in ("extract(epoch from ts_us)", "extract(millisecond from ts_us)", "extract(century from d)", "date_part(s, ts_us)", "date_part(1, ts_us)",
                "date_trunc('millennium', ts_us)", "date_trunc(s, ts_us)", "date_trunc('doy', ts_us)", "date_part('', d)"):
        assert describe(sql)[0] == NOT_SUPPORTED, sql
    for sql in ("date_part('year')", "date_part('year', d, d)", "date_trunc()", "date_trunc('day', ts_us, 1)"):
        assert describe(sql)[0] == INVALID_ARGUMENT, sql
    assert describe("extract(year from nope)")[0] == describe("nope")[0] != 0
    assert describe("extract(year from case when b then d else d2 end)")[0] == NOT_SUPPORTED
    # the names that were unknown stay unknown
    for name in ("abs", "foo", "concat", "now", "current_date", "date", "year"):
        assert describe(f"{name}(id)")[0] == NOT_IMPLEMENTED, name


def test_composition_types():
    head, lines = temporal_lines("date_trunc('day', ts_us) >= DATE '2024-03-01'")
    assert head == "result Boolean scalar=0 len1=0" and lines == ["trunc day kind=4 format=tsu:"]            # once, not twice
    assert temporal_lines("DATE '2024-03-01' > date_trunc('week', d)")[1] == ["trunc week kind=0 format=tdD"]
    assert temporal_lines("date_trunc('month', ts_us) = date_trunc('month', ts_us2)")[1] == ["trunc month kind=4 format=tsu:"] * 2
    assert temporal_lines("date_trunc('month', ts_us) < ts_us2")[1] == ["trunc month kind=4 format=tsu:"]
    assert temporal_lines("extract(year from date_trunc('quarter', ts_us))") == ("result Int32 scalar=0 len1=0", ["part year kind=4", "trunc quarter kind=4 format=tsu:"])
    assert temporal_lines("date_trunc('year', date_trunc('month', d))")[1] == ["trunc month kind=0 format=tdD", "trunc year kind=0 format=tdD"]      # operands first
    # (the operand of IN is typed once: one node, however many `=` read it, listed once and evaluated once)
    assert temporal_lines("extract(year from ts_us) = 2024 and extract(dow from ts_us) in (0, 6)")[1] == ["part year kind=4", "part dow kind=4"]
    # .. and so is a date_trunc under BETWEEN and IN: every comparison reads the one integer-typed copy of the node
    assert temporal_lines("date_trunc('day', ts_us) between DATE '2024-01-01' and DATE '2024-02-01'")[1] == ["trunc day kind=4 format=tsu:"]
    assert temporal_lines("date_trunc('day', ts_us) not between TIMESTAMP '2024-01-01 00:00' and ts_us2")[1] == ["trunc day kind=4 format=tsu:"]
    assert temporal_lines("date_trunc('month', d) in (DATE '2024-01-01', DATE '2024-02-01', DATE '2024-03-01')")[1] == ["trunc month kind=0 format=tdD"]
    assert temporal_lines("date_trunc('month', d) not in (DATE '2024-01-01', DATE '2024-02-01')")[1] == ["trunc month kind=0 format=tdD"]
    code, out = describe("case when extract(month from ts_us) < 7 then 1 else 2 end")
    assert code == 0 and "case whens=1 else=1 type=Int32 guarded=0" in out and "temporal part month kind=4" in out      # never a checked node
    code, out = describe("case when b then id + 1 else extract(year from d) end")
    assert code == 0 and "guarded=1" in out
    code, out = describe("cast(extract(year from ts_us) as bigint) * 100 + extract(month from ts_us)")
    assert code == 0 and out.startswith("result Int64 scalar=0 len1=0\n") and "temporal part year kind=4\ntemporal part month kind=4\n" in out and "cast Int32 -> Int64" in out
    code, out = describe("coalesce(date_trunc('day', d), d2)")
    assert code == 0 and "type=FixedWidth" in out and "temporal trunc day kind=0 format=tdD" in out
    # different DataTypes still do not compare; arithmetic keeps its answers; CASE results keep today's refusal and message
    assert describe("date_trunc('day', ts_us) = ts_ms")[0] == COERSION == describe("date_trunc('day', ts_us) = d")[0]
    assert describe("date_trunc('day', ts_us) >= TIMESTAMP '2024-03-01 00:00:00.0000001'")[0] == CAST_ERROR
    assert describe("date_trunc('day', d) >= TIMESTAMP '2024-03-01 00:00'")[0] == NOT_SUPPORTED
    assert describe("date_trunc('day', ts_us) - ts_us")[0] == describe("ts_us - ts_us2")[0] != 0
    assert describe("date_trunc('day', ts_us) * ts_us")[0] == describe("ts_us * ts_us2")[0] == INVALID_ARGUMENT
    code, out = describe("coalesce(d, d2) < d")
    assert code == NOT_SUPPORTED and out.endswith("an operator on the temporal / decimal result of CASE, coalesce or nullif is outside this build's scope")
    assert describe("coalesce(d, d2) < DATE '2024-01-01'") == (code, out)
    assert describe("date_trunc('day', ts_us) + 1")[0] == describe("ts_us + 1")[0] != 0


# ---- the per-row rules alone, under the sanitizers ---------------------------------------------------------------------------------------
N_EVERY = 2000      # per kind: the edge table and the first N_EVERY random values take every field and every unit;
#                     each of the N_RANDOM random values takes one field and one unit in turn


def sanitizer_cases():
    lines = []
    show = lambda v: "null" if v is None else str(v)
    for kind, K in R.KINDS.items():
        rand = R.random_values(kind, N_RANDOM)
        values = R.edges(kind) + rand[:N_EVERY]
        fields = [(fi, f) for fi, f in enumerate(R.FIELDS) if not K.is_time or f in R.TIME_FIELDS]
        units = [] if K.is_time else list(enumerate(R.UNITS))
        for fi, field in fields:
            lines += [f"part {K.code} {fi} {v} {show(R.part(kind, field, v))}" for v in values]
        for ui, unit in units:
            lines += [f"trunc {K.code} {ui} {v} {show(R.trunc(kind, unit, v))}" for v in values]
        for i, v in enumerate(rand):
            fi, field = fields[i % len(fields)]
            lines.append(f"part {K.code} {fi} {v} {show(R.part(kind, field, v))}")
            if units:
                ui, unit = units[i % len(units)]
                lines.append(f"trunc {K.code} {ui} {v} {show(R.trunc(kind, unit, v))}")
    word = {R.BAD: "bad", R.FINER: "finer", R.RANGE: "range"}
    for text, is_ts in GOOD + BAD + [("2300-01-01 00:00:00", True), ("1600-01-01 00:00:00", True), ("2262-04-11 23:47:16.854775807", True),
                                     ("2262-04-11 23:47:16.854775808", True), ("1677-09-21 00:12:43.145224192", True), ("1677-09-21 00:12:43.145224191", True)]:
        for kind in R.DATE_KINDS:
            want = R.literal_raw(is_ts, text, kind)
            lines.append(f"lit {int(is_ts)} {R.KINDS[kind].code} {text.encode().hex() or '-'} {word.get(want, want)}")
    return lines


def test_row_functions_under_host_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler on PATH")
    exe = str(tmp_path / "temporal_main")
    flags = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    src = os.path.join(ROOT, "tests", "temporal_main.cpp")
    build = subprocess.run([cxx, *flags, "-static-libasan", "-static-libubsan", src, "-o", exe], capture_output=True, text=True)
    if build.returncode != 0:
        build = subprocess.run([cxx, *flags, src, "-o", exe], capture_output=True, text=True)
    if build.returncode != 0 and re.search(r"asan|ubsan|sanitize", build.stderr, re.I):
        pytest.skip("the compiler has no sanitizer runtime: " + build.stderr.strip().splitlines()[-1])
    assert build.returncode == 0, build.stderr
    lines = sanitizer_cases()
    assert len(lines) > 6 * 2 * N_RANDOM + 4 * N_RANDOM
    cases = tmp_path / "cases.txt"
    cases.write_text("\n".join(lines) + "\n")
    run = subprocess.run([exe, str(cases)], capture_output=True, text=True)
    if run.returncode != 0 and "runtime does not come first" in run.stderr:
        pytest.skip("this environment preloads a library in front of the sanitizer runtime: " + run.stderr.strip().splitlines()[0])
    assert run.returncode == 0, run.stdout + run.stderr[-4000:]
    assert run.stdout.startswith(f"{len(lines)} cases, 0 mismatches"), run.stdout


# ---- the round size of tests/test_gpu_temporal.py, held to the sources ---------------------------------------------------------------------
def test_round_sizes_of_the_gpu_tests():
    from . import test_gpu_temporal as G
    header = open(os.path.join(CSRC, "temporal_device.h")).read()
    kernels = open(os.path.join(CSRC, "temporal.hip")).read()
    shared, grid = (open(os.path.join(CSRC, name)).read() for name in ("wave_rows.h", "typed_ops.h"))
    cap = int(eval(re.search(r"constexpr\s+int\s+TEMPORAL_GRID_CAP\s*=\s*([\d *]+);", header).group(1)))
    block = int(re.search(r"constexpr int kRowsBlock = (\d+);", shared).group(1))
    assert block == 256 and grid.count("inline unsigned rows_grid(int64_t items, int64_t cap_blocks) {") == 1
    # both kernels are on the shared row loop and epilogue, in workgroups of kRowsBlock threads, on the capped grid
    assert kernels.count("CHQ_FOR_WAVE_ROWS(base, nrows) {\n    const int64_t i = base + lane_id();") == 2 == kernels.count("CHQ_FOR_WAVE_ROWS")
    assert kernels.count("__launch_bounds__(kRowsBlock)") == 2 and kernels.count("store_validity_word(p.out_validity, p.null_count, base, wave_rows_end(nrows, base), __ballot(valid));") == 2
    assert kernels.count("const dim3 grid(rows_grid(p.nrows, TEMPORAL_GRID_CAP)), block(kRowsBlock);") == 2 and "gridDim" not in kernels and "blockIdx" not in kernels
    launches = re.findall(r"hipLaunchKernelGGL\(\((\w+)<K>\), grid, block, 0, stream, p\)", kernels)
    assert launches == ["temporal_part_kernel", "temporal_trunc_kernel"] and kernels.count("hipLaunchKernelGGL(") == 2
    assert "atomic" not in re.sub(r"//[^\n]*", "", kernels)      # (the one atomic per wave is store_validity_word's)
    assert G.GRID_ROWS == cap * block and G.SECOND_ROUND_ROWS == G.GRID_ROWS + 65
