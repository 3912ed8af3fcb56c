"""GPU: DATE / TIMESTAMP literals, EXTRACT / date_part and date_trunc on the device (temporal.hip).  Every result goes through the
C ABI and is compared -- values, validity, null count, type -- with tests/temporal_reference.py, which the CPU tier pins to pyarrow
and `datetime`.  Columns are built from raw buffers, so that null slots can hold values outside the calendar's range."""
import numpy as np
import pyarrow as pa
import pytest

import chapterhouseqe_amd as chq
from chapterhouseqe_amd import sqlast as A
from chapterhouseqe_amd.sqlparse import parse_expr, parse_select

from . import temporal_reference as R
from .cases import empty_aliases

pytestmark = pytest.mark.gpu

# held to the sources by tests/test_temporal_host.py::test_round_sizes_of_the_gpu_tests
GRID_ROWS = 256 * 32 * 256            # rows one round of the capped grid of temporal.hip covers
SECOND_ROUND_ROWS = GRID_ROWS + 65    # the second round runs, with a partial last wave
ROW_COUNTS = (1, 63, 64, 65, 127, 129)


@pytest.fixture(scope="module")
def ctx():
    c = chq.Context(0)
    yield c
    c.close()


# ---- columns from raw buffers ---------------------------------------------------------------------------------------------------
def np_dtype(kind):
    return np.int32 if R.KINDS[kind].bits == 32 else np.int64


def column(values, valid, kind, arrow=None):
    """an Arrow array of the kind's type from raw values; a null slot keeps ITS value in the buffer"""
    n = len(values)
    valid = np.asarray(valid, bool)
    nulls = int(n - np.count_nonzero(valid))
    bm = pa.py_buffer(np.packbits(valid, bitorder="little").tobytes()) if nulls else None
    return pa.Array.from_buffers(arrow or R.KINDS[kind].arrow, n, [bm, pa.py_buffer(np.asarray(values, np_dtype(kind)).tobytes())], null_count=nulls)


def batch_of(values, valid, kind, name="x", arrow=None):
    return pa.RecordBatch.from_arrays([column(values, valid, kind, arrow)], names=[name])


def check_array(arr, want, valid, typ, dtype, what):
    """`arr` (a host array read back) against the reference's (values, validity): type, null count, bitmap, the values of the
    valid rows, and the zeroes the kernels write into null rows"""
    n = len(want)
    assert arr.type == typ and len(arr) == n and arr.offset == 0, (what, arr.type, len(arr))
    vmask = np.asarray(valid, bool)
    nulls = int(n - np.count_nonzero(vmask))
    assert arr.null_count == nulls, (what, arr.null_count, nulls)
    bufs = arr.buffers()
    if nulls:
        got_valid = np.unpackbits(np.frombuffer(bufs[0], np.uint8), bitorder="little")[:n].astype(bool)
        bad = np.flatnonzero(got_valid != vmask)[:8]
        assert not len(bad), f"{what}: validity differs first at rows {bad.tolist()}"
    else:
        assert bufs[0] is None, what
    got = np.frombuffer(bufs[1], dtype, n)
    exp = np.where(vmask, np.asarray(want, dtype), 0).astype(dtype)
    bad = np.flatnonzero(got != exp)[:8]
    assert not len(bad), f"{what}: values differ first at rows {bad.tolist()}: got {got[bad].tolist()} expected {exp[bad].tolist()}"


def run(c, rec, expr, host=None):
    arr, is_scalar = chq.compute_value(rec, empty_aliases(host if host is not None else rec), parse_expr(expr) if isinstance(expr, str) else expr, ctx=c)
    assert not is_scalar
    return arr


def host_of(b):
    return b.to_host() if hasattr(b, "to_host") else b


def fields_of(kind):
    return R.TIME_FIELDS if R.KINDS[kind].is_time else R.FIELDS


def check_op(c, rec, host, kind, op, name, values, valid, what, arrow=None):
    """one EXTRACT (op = 'part') or date_trunc (op = 'trunc') over a batch against the reference"""
    if op == "part":
        want, wvalid = R.part_rows(kind, name, values, valid)
        check_array(run(c, rec, f"extract({name} from x)", host), want, wvalid, pa.int32(), np.int32, what)
    else:
        want, wvalid = R.trunc_rows(kind, name, values, valid)
        check_array(run(c, rec, f"date_trunc('{name}', x)", host), want, wvalid, arrow or R.KINDS[kind].arrow, np_dtype(kind), what)


# ---- every (source type x field) and (source type x unit) over the whole edge table -----------------------------------------------
@pytest.mark.parametrize("kind", list(R.KINDS))
def test_every_field_and_unit_over_the_edge_table(ctx, kind):
    K = R.KINDS[kind]
    table = R.edges(kind)
    # (Int64 nanoseconds hold no date outside the year range: their nulls are the truncations that do not fit)
    assert (kind == "ts_ns" or any(R.split(kind, v) is None for v in table)) and any(R.split(kind, v) is not None for v in table)
    for nullable in (False, True):
        values = list(table)
        valid = [True] * len(values)
        if nullable:      # every third slot is null and holds out-of-range garbage, which is never judged
            valid = [i % 3 != 1 for i in range(len(values))]
            values = [v if ok else (K.lo if i % 2 else K.hi) for i, (v, ok) in enumerate(zip(values, valid))]
        host = batch_of(values, valid, kind)
        dev = chq.DeviceRecordBatch.from_host(host, ctx)
        for rec in (dev, host):      # device-resident and host-resident input
            for field in fields_of(kind):
                check_op(ctx, rec, host, kind, "part", field, values, valid, f"{kind} {field} nullable={nullable} device={rec is dev}")
            for unit in (() if K.is_time else R.UNITS):
                check_op(ctx, rec, host, kind, "trunc", unit, values, valid, f"{kind} trunc {unit} nullable={nullable} device={rec is dev}")


def test_rows_the_null_rule_makes_null_are_counted(ctx):
    """no input null, yet the result holds nulls: they land in the validity words and in the exported null count"""
    for kind in ("date32", "ts_s", "ts_ns"):
        K = R.KINDS[kind]
        values = [0, K.lo, 1, K.hi, -1, K.lo + 1] * 40
        host = batch_of(values, [True] * len(values), kind)
        arr = run(ctx, host, "extract(year from x)")
        want, wvalid = R.part_rows(kind, "year", values, [True] * len(values))
        assert arr.null_count == wvalid.count(False) and arr.to_pylist() == [w if ok else None for w, ok in zip(want, wvalid)]
        arr = run(ctx, host, "date_trunc('day', x)")
        want, wvalid = R.trunc_rows(kind, "day", values, [True] * len(values))
        assert arr.null_count == wvalid.count(False) > 0 and arr.type == K.arrow
    # Timestamp(ns): the first day of Int64 has a year but no day floor
    assert R.part("ts_ns", "year", R.KINDS["ts_ns"].lo) == 1677 and R.trunc("ts_ns", "day", R.KINDS["ts_ns"].lo) is None


# ---- row counts: the bitmap words; the second round of the capped grid ----------------------------------------------------------------
def cycled(table, n):
    return [table[i % len(table)] for i in range(n)]


@pytest.mark.parametrize("n", ROW_COUNTS)
def test_row_counts(ctx, n):
    for kind, op, name in (("ts_us", "part", "year"), ("ts_s", "part", "week"), ("date32", "trunc", "week"), ("ts_ns", "trunc", "day"),
                           ("date64", "trunc", "month"), ("time32_s", "part", "minute"), ("time64_ns", "part", "second"), ("ts_ms", "part", "doy")):
        values = cycled(R.edges(kind), n)
        for valid in ([True] * n, [i % 3 != 1 for i in range(n)]):
            host = batch_of(values, valid, kind)
            check_op(ctx, host, host, kind, op, name, values, valid, f"{kind} {op} {name} n={n}")
            check_op(ctx, chq.DeviceRecordBatch.from_host(host, ctx), host, kind, op, name, values, valid, f"{kind} {op} {name} n={n} device")


@pytest.mark.parametrize("kind,op,name", [("ts_us", "part", "year"), ("ts_us", "trunc", "month"), ("date32", "part", "week"), ("date32", "trunc", "quarter")])
def test_second_round_of_the_capped_grid(ctx, kind, op, name):
    n = SECOND_ROUND_ROWS
    table = R.edges(kind)
    if len(table) % 2 == 0:      # an odd period is coprime to 64: every table entry meets every lane
        table = table[:-1]
    idx = np.arange(n) % len(table)
    ones = [True] * len(table)
    want_t, valid_t = (R.part_rows if op == "part" else R.trunc_rows)(kind, name, table, ones)
    assert not all(valid_t)
    vals = np.asarray(table, np_dtype(kind))[idx]
    host = pa.RecordBatch.from_arrays([pa.Array.from_buffers(R.KINDS[kind].arrow, n, [None, pa.py_buffer(vals.tobytes())], null_count=0)], names=["x"])
    dev = chq.DeviceRecordBatch.from_host(host, ctx)
    arr = run(ctx, dev, f"extract({name} from x)" if op == "part" else f"date_trunc('{name}', x)", host)
    out_dtype = np.int32 if op == "part" else np_dtype(kind)
    check_array(arr, np.asarray(want_t, out_dtype)[idx], np.asarray(valid_t, bool)[idx], pa.int32() if op == "part" else R.KINDS[kind].arrow, out_dtype,
                f"{kind} {op} {name} over {n} rows")


# ---- sliced views: values and validity read from an element / bit offset -----------------------------------------------------------------
@pytest.mark.parametrize("off", (1, 7, 63, 65))
def test_sliced_views(ctx, off):
    n = 200
    for kind, op, name in (("date32", "part", "doy"), ("date32", "trunc", "month"), ("ts_us", "part", "week"), ("ts_us", "trunc", "hour"), ("ts_s", "part", "dow"),
                           ("time32_ms", "part", "hour")):
        values = cycled(R.edges(kind), n + off + 3)
        for valid in ([True] * len(values), [i % 3 != 2 for i in range(len(values))]):
            host = batch_of(values, valid, kind)
            view = chq.DeviceRecordBatch.from_host(host, ctx).slice(off, n)
            check_op(ctx, view, host, kind, op, name, values[off:off + n], valid[off:off + n], f"{kind} {op} {name} view at {off}")
            check_op(ctx, host.slice(off, n), None, kind, op, name, values[off:off + n], valid[off:off + n], f"{kind} {op} {name} host slice at {off}")


# ---- literal comparisons: the integer comparison of the raw values ------------------------------------------------------------------------
LITERAL_COLUMNS = [("date32", None, False, "2024-03-01"), ("date64", None, False, "2024-03-01"), ("ts_s", None, True, "2024-03-01 12:00:00"),
                   ("ts_ms", None, True, "2024-03-01 12:00:00.250"), ("ts_us", None, True, "2024-03-01T12:00"), ("ts_ns", None, True, "2024-03-01 12:00:00.000000001"),
                   ("ts_us", pa.timestamp("us", "UTC"), False, "2024-03-01")]
OPS = {"=": np.equal, "<>": np.not_equal, "<": np.less, "<=": np.less_equal, ">": np.greater, ">=": np.greater_equal}
MIRROR = {"=": "=", "<>": "<>", "<": ">", "<=": ">=", ">": "<", ">=": "<="}


def literal_batch(kind, arrow, raw, n=130):
    """raw values around the literal's, an id column, every fifth row null"""
    K = R.KINDS[kind]
    step = K.per_day or 1
    values = [raw + d for d in (0, 1, -1, step, -step, 1000 * step)] + [0, K.lo, K.hi]
    values = cycled(values, n)
    valid = [i % 5 != 3 for i in range(n)]
    return pa.RecordBatch.from_arrays([column(values, valid, kind, arrow), pa.array(np.arange(n, dtype=np.int32))], names=["x", "id"]), values, valid


@pytest.mark.parametrize("kind,arrow,is_ts,text", LITERAL_COLUMNS)
def test_literal_comparisons_through_every_entry(ctx, kind, arrow, is_ts, text):
    raw = R.literal_raw(is_ts, text, kind)
    lit = f"{'TIMESTAMP' if is_ts else 'DATE'} '{text}'"
    host, values, valid = literal_batch(kind, arrow, raw)
    others = [literal_batch(kind, arrow, raw, n)[0] for n in (1, 65)]
    dev = chq.DeviceRecordBatch.from_host(host, ctx)
    vals, vmask = np.asarray(values, np.int64), np.asarray(valid, bool)
    ids = np.arange(len(values))
    for op, fn in OPS.items():
        truth = fn(vals, raw)
        for sql in (f"x {op} {lit}", f"{lit} {MIRROR[op]} x"):      # both orders
            expr = parse_expr(sql)
            want = [bool(t) if ok else None for t, ok in zip(truth, valid)]
            assert run(ctx, dev, expr, host).to_pylist() == want == run(ctx, host, expr).to_pylist(), sql
            kept = ids[truth & vmask].tolist()
            for rec in (dev, host):
                assert host_of(chq.filter_record(rec, empty_aliases(host), expr, ctx=ctx)).column("id").to_pylist() == kept, sql
            outs = chq.filter_records([host] + others, empty_aliases(host), expr, ctx=ctx)
            assert len(outs) == 3 and host_of(outs[0]).column("id").to_pylist() == kept, sql
            for o, rec in zip(outs[1:], others):
                n = rec.num_rows
                assert host_of(o).column("id").to_pylist() == ids[:n][truth[:n] & vmask[:n]].tolist(), sql
            got = host_of(chq.project_record(parse_select(f"select {sql} as k, id from t").projection, dev, empty_aliases(host), ctx=ctx))
            assert got.column("k").to_pylist() == want and got.column("id").to_pylist() == ids.tolist(), sql
    # BETWEEN and IN are comparisons
    step = R.KINDS[kind].per_day or 1
    day_after = "2024-03-02" + text[10:]
    hi = R.literal_raw(is_ts, day_after, kind)
    assert hi == raw + step
    word = "TIMESTAMP" if is_ts else "DATE"
    between = ((vals >= raw) & (vals <= hi))
    assert run(ctx, dev, f"x between {lit} and {word} '{day_after}'", host).to_pylist() == [bool(t) if ok else None for t, ok in zip(between, valid)]
    assert run(ctx, dev, f"x not between {lit} and {word} '{day_after}'", host).to_pylist() == [bool(not t) if ok else None for t, ok in zip(between, valid)]
    member = (vals == raw) | (vals == hi)
    assert run(ctx, dev, f"x in ({lit}, {word} '{day_after}')", host).to_pylist() == [bool(t) if ok else None for t, ok in zip(member, valid)]
    kept = host_of(chq.filter_record(dev, empty_aliases(host), parse_expr(f"x not in ({lit}, {word} '{day_after}')"), ctx=ctx)).column("id").to_pylist()
    assert kept == ids[~member & vmask].tolist()


# ---- composition ---------------------------------------------------------------------------------------------------------------------
def events(n=3000, seed=11, tz=None):
    """Timestamp(us) over 2023-2025 and a Date32 column, with nulls; (batch, raw ts, ts validity, raw d)"""
    rng = np.random.default_rng(seed)
    lo, hi = R.days_from_civil(2023, 1, 1) * 86400 * 10**6, R.days_from_civil(2025, 12, 31) * 86400 * 10**6
    ts = rng.integers(lo, hi, n, dtype=np.int64)
    ts[:4] = [R.literal_raw(True, t, "ts_us") for t in ("2024-03-01 00:00:00", "2024-02-29 23:59:59.999999", "2024-12-29 12:00:00", "2023-12-31 23:59:59")]
    d = rng.integers(R.days_from_civil(1999, 1, 1), R.days_from_civil(2030, 1, 1), n, dtype=np.int64).astype(np.int32)
    valid = [i % 11 != 5 for i in range(n)]
    rec = pa.RecordBatch.from_arrays([column(ts, valid, "ts_us", pa.timestamp("us", tz)), column(d, [True] * n, "date32"), pa.array(np.arange(n, dtype=np.int32))],
                                     names=["ts", "d", "id"])
    return rec, ts.tolist(), valid, d.tolist()


def test_where_and_select_compositions(ctx):
    rec, ts, valid, d = events()
    dev = chq.DeviceRecordBatch.from_host(rec, ctx)
    al = empty_aliases(rec)
    part = lambda f: [R.part("ts_us", f, v) if ok else None for v, ok in zip(ts, valid)]
    year, dow, month = part("year"), part("dow"), part("month")
    for src in (dev, rec):
        got = host_of(chq.filter_record(src, al, parse_expr("extract(year from ts) = 2024 and extract(dow from ts) in (0, 6)"), ctx=ctx))
        assert got.column("id").to_pylist() == [i for i in range(len(ts)) if year[i] == 2024 and dow[i] in (0, 6)]
        bound = R.literal_raw(False, "2024-03-01", "ts_us")
        got = host_of(chq.filter_record(src, al, parse_expr("date_trunc('day', ts) >= DATE '2024-03-01'"), ctx=ctx))
        assert got.column("id").to_pylist() == [i for i in range(len(ts)) if valid[i] and R.trunc("ts_us", "day", ts[i]) >= bound]
        assert got.schema == rec.schema
        got = host_of(chq.project_record(parse_select("select date_trunc('month', ts) m, extract(doy from d) n from t").projection, src, al, ctx=ctx))
        want_m, mvalid = R.trunc_rows("ts_us", "month", ts, valid)
        check_array(got.column("m"), want_m, mvalid, pa.timestamp("us"), np.int64, "select date_trunc('month', ts)")
        assert got.column("n").equals(pa.array([R.part("date32", "doy", v) for v in d], pa.int32())) and got.schema.names == ["m", "n"]
        assert [f.nullable for f in got.schema] == [True, False]
        arr = run(ctx, src, "case when extract(month from ts) < 7 then 1 else 2 end", rec)
        assert arr.to_pylist() == [(1 if m < 7 else 2) if m is not None else 2 for m in month]      # (a NULL condition is not true)
        arr = run(ctx, src, "cast(extract(year from ts) as bigint) * 100 + extract(month from ts)", rec)
        assert arr.type == pa.int64() and arr.to_pylist() == [None if y is None else y * 100 + m for y, m in zip(year, month)]
        arr = run(ctx, src, "extract(hour from date_trunc('day', ts))", rec)
        assert arr.to_pylist() == [0 if ok else None for ok in valid]
        arr = run(ctx, src, "extract(year from date_trunc('quarter', ts)) = extract(year from ts)", rec)
        assert arr.to_pylist() == [True if ok else None for ok in valid]
        arr = run(ctx, src, "date_trunc('month', ts) = date_trunc('month', ts)", rec)
        assert arr.to_pylist() == [True if ok else None for ok in valid]
        arr = run(ctx, src, "date_trunc('month', ts) < ts", rec)
        assert arr.to_pylist() == [R.trunc("ts_us", "month", v) < v if ok else None for v, ok in zip(ts, valid)]
        arr = run(ctx, src, "date_part('WEEK', d) + date_part('dow', d)", rec)
        assert arr.to_pylist() == [R.part("date32", "week", v) + R.part("date32", "dow", v) for v in d]


def test_date_trunc_keeps_the_operands_format(ctx):
    for tz in (None, "UTC", "+00:00"):
        rec, ts, valid, _ = events(300, 5, tz)
        want, wvalid = R.trunc_rows("ts_us", "week", ts, valid)
        for src in (rec, chq.DeviceRecordBatch.from_host(rec, ctx)):
            check_array(run(ctx, src, "date_trunc('week', ts)", rec), want, wvalid, pa.timestamp("us", tz), np.int64, f"zone {tz}")
            got = host_of(chq.project_record(parse_select("select date_trunc('week', ts) w, coalesce(date_trunc('day', ts), ts) c from t").projection, src, empty_aliases(rec), ctx=ctx))
            assert got.schema.field("w").type == pa.timestamp("us", tz) == got.schema.field("c").type
        if tz:      # the literal beside a UTC column is UTC
            bound = R.literal_raw(True, "2024-03-01 00:00:00", "ts_us")
            arr = run(ctx, rec, "ts >= TIMESTAMP '2024-03-01 00:00:00'")
            assert arr.to_pylist() == [v >= bound if ok else None for v, ok in zip(ts, valid)]
    for kind in ("date32", "date64", "ts_s", "ts_ms", "ts_ns"):
        host = batch_of(R.edges(kind)[:20], [True] * 20, kind)
        assert run(ctx, host, "date_trunc('year', x)").type == R.KINDS[kind].arrow


def test_a_date_trunc_result_as_sort_and_group_key(ctx):
    """two calls, no new operator code: a projection in front, then ORDER BY / GROUP BY on its temporal column"""
    rec, ts, valid, _ = events(2000, 3)
    dev = chq.DeviceRecordBatch.from_host(rec, ctx)
    proj = chq.project_record(parse_select("select date_trunc('month', ts) m, id from t").projection, dev, empty_aliases(rec), ctx=ctx)
    months = [R.trunc("ts_us", "month", v) if ok else None for v, ok in zip(ts, valid)]
    al = [[], []]
    got = host_of(chq.sort_record(proj, al, [A.OrderByExpr(A.ident("m")), A.OrderByExpr(A.ident("id"))], ctx=ctx))
    order = sorted(range(len(ts)), key=lambda i: (months[i] is None, months[i] or 0, i))      # ascending, nulls last, stable
    assert got.column("id").to_pylist() == order and got.schema.field("m").type == pa.timestamp("us")
    agg = host_of(chq.aggregate_record(proj, al, [A.ident("m")], [A.AggItem(A.AggKind.KEY, "m", 0), A.AggItem(A.AggKind.COUNT_STAR, "n")], ctx=ctx))
    groups = {}
    for m in months:
        groups[m] = groups.get(m, 0) + 1
    keys = sorted((k for k in groups if k is not None)) + ([None] if None in groups else [])
    assert agg.column("m").cast(pa.int64()).to_pylist() == keys and agg.column("n").to_pylist() == [groups[k] for k in keys]
    assert len(keys) == 37 and agg.schema.field("m").type == pa.timestamp("us")


def test_launch_accounting(ctx):
    rec, ts, valid, _ = events(5000, 9)
    dev = chq.DeviceRecordBatch.from_host(rec, ctx)
    al = empty_aliases(rec)
    n = rec.num_rows
    chq.filter_record(dev, al, parse_expr("ts >= TIMESTAMP '2024-03-01 00:00:00'"), ctx=ctx)
    plain = ctx.last_stats()
    chq.filter_record(dev, al, parse_expr("date_trunc('day', ts) >= DATE '2024-03-01'"), ctx=ctx)
    with_trunc = ctx.last_stats()
    # one launch of the truncation kernel on top of the filter's own: the literal did not make the operand run twice
    assert with_trunc["launches"] == plain["launches"] + 1, (plain, with_trunc)
    words = (n + 7) // 8
    assert with_trunc["bytes_read_alg"] - plain["bytes_read_alg"] >= n * 8 + words and with_trunc["bytes_written_alg"] - plain["bytes_written_alg"] >= n * 8 + words
    chq.compute_value(dev, al, parse_expr("date_trunc('month', ts) = date_trunc('year', ts)"), ctx=ctx)
    two = ctx.last_stats()
    chq.compute_value(dev, al, parse_expr("ts = ts"), ctx=ctx)
    assert two["launches"] == ctx.last_stats()["launches"] + 2
    # a date_trunc under BETWEEN and IN is one node read by every comparison: one launch of the truncation kernel, and the reference's rows
    days = [R.trunc("ts_us", "day", v) if ok else None for v, ok in zip(ts, valid)]
    lo, hi, third = (R.literal_raw(False, t, "ts_us") for t in ("2024-03-01", "2024-03-31", "2024-12-29"))
    ids = list(range(n))
    for sql, ref_sql, keep in (
            ("date_trunc('day', ts) between DATE '2024-03-01' and DATE '2024-03-31'", "ts between TIMESTAMP '2024-03-01 00:00' and TIMESTAMP '2024-03-31 00:00'",
             lambda t: lo <= t <= hi),
            ("date_trunc('day', ts) not between DATE '2024-03-01' and DATE '2024-03-31'", "ts not between TIMESTAMP '2024-03-01 00:00' and TIMESTAMP '2024-03-31 00:00'",
             lambda t: not lo <= t <= hi),
            ("date_trunc('day', ts) in (DATE '2024-03-01', DATE '2024-03-31', DATE '2024-12-29')",
             "ts in (TIMESTAMP '2024-03-01 00:00', TIMESTAMP '2024-03-31 00:00', TIMESTAMP '2024-12-29 00:00')", lambda t: t in (lo, hi, third)),
            ("date_trunc('day', ts) not in (DATE '2024-03-01', DATE '2024-03-31', DATE '2024-12-29')",
             "ts not in (TIMESTAMP '2024-03-01 00:00', TIMESTAMP '2024-03-31 00:00', TIMESTAMP '2024-12-29 00:00')", lambda t: t not in (lo, hi, third))):
        got = chq.filter_record(dev, al, parse_expr(sql), ctx=ctx)
        st = ctx.last_stats()
        assert host_of(got).column("id").to_pylist() == [i for i in ids if days[i] is not None and keep(days[i])], sql
        chq.filter_record(dev, al, parse_expr(ref_sql), ctx=ctx)      # the same comparisons on the column itself
        assert st["launches"] == ctx.last_stats()["launches"] + 1, (sql, st)
    chq.compute_value(dev, al, parse_expr("extract(dow from ts) in (0, 6)"), ctx=ctx)      # the operand of IN is evaluated once
    one = ctx.last_stats()
    chq.compute_value(dev, al, parse_expr("id in (0, 6)"), ctx=ctx)
    assert one["launches"] == ctx.last_stats()["launches"] + 1
