"""GPU: CAST / TRY_CAST on the device (cast.hip).  Every result goes through the C ABI and is compared buffer by buffer (values,
validity, offsets, null count, nullability) and bit for bit with tests/cast_reference.py, which the CPU tier pins to pyarrow and
sqlite3.  Columns are built from raw buffers, so that null slots can hold values that would fail."""
import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest

import chapterhouseqe_amd as chq
from chapterhouseqe_amd import sqlast as A
from chapterhouseqe_amd.sqlparse import parse_expr, parse_select

from . import cast_reference as R
from . import float_reference as F
from . import int_reference as I
from .cases import empty_aliases

pytestmark = pytest.mark.gpu

# held to the sources by tests/test_cast_host.py::test_round_sizes_of_the_gpu_tests
GRID_ROWS = 256 * 16 * 256          # rows one round of a capped grid of cast.hip covers
SCAN_TILE = 2048                    # rows per tile of the offsets scan
SCAN_ROUND = 256 * SCAN_TILE        # rows one round of the scan of the tile totals covers
ROW_COUNTS = (0, 1, 63, 64, 65, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1)
SECOND_ROUND_ROWS = GRID_ROWS + 1   # the smallest count whose last row belongs to the second round


@pytest.fixture(scope="module")
def ctx():
    c = chq.Context(0)
    yield c
    c.close()


# ---- columns from raw buffers -------------------------------------------------------------------------------------------------
def bitmap_of(valid):
    valid = np.asarray(valid, bool)
    return None if valid.all() else pa.py_buffer(np.packbits(valid, bitorder="little").tobytes())


def column(values, valid, typ):
    """an Arrow array of `typ` from the reference's values; a null slot keeps ITS value in the buffers"""
    n = len(values)
    nulls = int(n - np.count_nonzero(valid))
    bm = bitmap_of(valid) if nulls else None
    if typ == "utf8":
        offs = np.zeros(n + 1, np.int64)
        np.cumsum([len(b) for b in values], out=offs[1:])
        return pa.Array.from_buffers(pa.utf8(), n, [bm, pa.py_buffer(offs.astype(np.int32).tobytes()), pa.py_buffer(b"".join(values))], null_count=nulls)
    if typ == "bool":
        return pa.Array.from_buffers(pa.bool_(), n, [bm, pa.py_buffer(np.packbits(np.asarray(values, bool), bitorder="little").tobytes())], null_count=nulls)
    dtype = F.FORMATS[typ].utype if typ in R.FLOATS else I.TYPES[typ].dtype
    return pa.Array.from_buffers(R.ARROW[typ], n, [bm, pa.py_buffer(np.array(values, dtype=dtype).tobytes())], null_count=nulls)


def batch_of(values, valid, typ, name="x"):
    return pa.RecordBatch.from_arrays([column(values, valid, typ)], names=[name])


def cast_expr(dst, try_cast, name="x"):
    return A.Cast(A.ident(name), A.CastType(R.CODE[dst]), try_cast)


def check_array(arr, want, valid, dst, what):
    """`arr` (a host array read back) against the reference's (values, validity)"""
    n = len(want)
    assert arr.type == R.ARROW[dst] and len(arr) == n and arr.offset == 0, (what, arr.type, len(arr))
    nulls = n - sum(valid)
    assert arr.null_count == nulls, (what, arr.null_count, nulls)
    bufs = arr.buffers()
    vmask = np.asarray(valid, bool)
    if nulls:
        got_valid = np.unpackbits(np.frombuffer(bufs[0], np.uint8), bitorder="little")[:n].astype(bool)
        bad = np.flatnonzero(got_valid != vmask)[:8]
        assert not len(bad), f"{what}: validity differs first at rows {bad.tolist()}"
    else:
        assert bufs[0] is None, what
    if n == 0:
        return
    if dst == "utf8":
        exp_offs = np.zeros(n + 1, np.int64)
        np.cumsum([len(w) for w in want], out=exp_offs[1:])
        offs = np.frombuffer(bufs[1], np.int32, n + 1)
        bad = np.flatnonzero(offs != exp_offs)[:8]
        assert not len(bad), f"{what}: offsets differ first at {bad.tolist()}: got {offs[bad].tolist()} expected {exp_offs[bad].tolist()}"
        total = int(exp_offs[-1])
        assert (bufs[2].to_pybytes()[:total] if total else b"") == b"".join(want), what
        return
    if dst == "bool":
        got = np.unpackbits(np.frombuffer(bufs[1], np.uint8), bitorder="little")[:n].astype(bool)
        exp = np.asarray(want, bool)
    else:
        dtype = F.FORMATS[dst].utype if dst in R.FLOATS else I.TYPES[dst].dtype
        got = np.frombuffer(bufs[1], dtype, n)
        exp = np.array(want, dtype=dtype)
    bad = np.flatnonzero((got != exp) & vmask)[:8]
    assert not len(bad), f"{what}: values differ first at rows {bad.tolist()}: got {got[bad].tolist()} expected {exp[bad].tolist()}"


def run(c, rec, expr, host=None):
    arr, is_scalar = chq.compute_value(rec, empty_aliases(host if host is not None else rec), expr, ctx=c)
    assert not is_scalar
    return arr


def expect_cast_error(c, rec, expr, src, dst, host=None):
    with pytest.raises(chq.ChqError) as ei:
        run(c, rec, expr, host)
    assert ei.value.code == R.CAST_ERROR and R.NAME[src] in str(ei.value) and R.NAME[dst] in str(ei.value), str(ei.value)


def spread_nulls(n, step=5, at=2):
    return [i % step != at for i in range(n)]


# ---- every pair over its edge table ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("src", R.ALL)
def test_every_pair_over_the_edge_tables(ctx, src):
    met = 0
    for dst in R.ALL:
        if src == dst or not R.supported(src, dst):
            continue
        clean, failing = R.clean_rows(src, dst), R.failing_rows(src, dst)
        assert len(clean) >= 2 and bool(failing) == R.can_fail(src, dst), (src, dst)
        for nulls in (False, True):
            # a table without a failing VALID row: CAST and TRY_CAST give the same column.  With nulls, the null slots hold
            # the failing values (failures are reported on valid rows only)
            values = list(clean)
            valid = [True] * len(values)
            if nulls:
                values = [v for pair in zip(clean, (failing or clean) * len(clean)) for v in pair][:2 * len(clean)]
                valid = [i % 2 == 0 for i in range(len(values))]
            want, wvalid, failed = R.cast_rows(values, valid, src, dst)
            assert failed is None
            dev = chq.DeviceRecordBatch.from_host(batch_of(values, valid, src), ctx)
            for try_cast in (False, True):
                check_array(run(ctx, dev, cast_expr(dst, try_cast), batch_of(values, valid, src)), want, wvalid, dst, f"{src}->{dst} try={try_cast} nulls={nulls}")
                met += 1
            if not failing:
                continue
            # a table with failing rows: CAST ends the call, TRY_CAST makes them null
            mixed = [v for pair in zip(clean * len(failing), failing) for v in pair][:2 * len(failing)] + clean[:3]
            mvalid = spread_nulls(len(mixed), 7, 3) if nulls else [True] * len(mixed)
            want, wvalid, failed = R.cast_rows(mixed, mvalid, src, dst)
            assert failed is not None
            host = batch_of(mixed, mvalid, src)
            dev = chq.DeviceRecordBatch.from_host(host, ctx)
            expect_cast_error(ctx, dev, cast_expr(dst, False), src, dst, host)
            check_array(run(ctx, dev, cast_expr(dst, True), host), want, wvalid, dst, f"{src}->{dst} try over failing rows nulls={nulls}")
            met += 1
    assert met >= 20


# ---- row counts: the bitmap words, the scan tile, the second round of the capped grids ----------------------------------------
def cycled(table, n):
    return [table[i % len(table)] for i in range(n)]


COUNT_PAIRS = [("i32", "i64"), ("i64", "i8"), ("i32", "utf8"), ("utf8", "i32"), ("f64", "i32"), ("bool", "i32"), ("i32", "bool"), ("bool", "utf8"),
               ("u64", "f32"), ("utf8", "bool")]


@pytest.mark.parametrize("n", ROW_COUNTS)
def test_row_counts(ctx, n):
    for src, dst in COUNT_PAIRS:
        values = cycled(R.bool_strings() if (src, dst) == ("utf8", "bool") else R.edges(src), n)
        for valid in ([True] * n, spread_nulls(n, 3, 1)):
            want, wvalid, _ = R.cast_rows(values, valid, src, dst)
            host = batch_of(values, valid, src)
            check_array(run(ctx, host, cast_expr(dst, True)), want, wvalid, dst, f"{src}->{dst} n={n}")      # (a host-resident batch)
            if n:
                dev = chq.DeviceRecordBatch.from_host(host, ctx)
                check_array(run(ctx, dev, cast_expr(dst, True), host), want, wvalid, dst, f"{src}->{dst} n={n} device")


def test_zero_rows_for_every_kind_of_typed_operation(ctx):
    """a device batch of no rows: every operator that becomes a temporary column (materialize.cpp) answers with an empty
    column of its type and no nulls, and a Boolean one filters to no rows"""
    host = pa.RecordBatch.from_arrays([pa.array([], pa.int32()), pa.array([], pa.utf8()), pa.array([], pa.bool_())], names=["id", "s", "b"])
    dev = chq.DeviceRecordBatch.from_host(host, ctx)
    for sql, typ in (("upper(s)", pa.utf8()), ("s || 'x'", pa.utf8()), ("length(s)", pa.int32()), ("s like 'a%'", pa.bool_()), ("s is null", pa.bool_()),
                     ("s and b", pa.bool_()), ("case when b then s else 'n' end", pa.utf8()), ("case when b then id else 0 end", pa.int32()),
                     ("cast(id as varchar)", pa.utf8()), ("cast(s as int)", pa.int32()), ("try_cast(s as boolean)", pa.bool_())):
        arr = run(ctx, dev, parse_expr(sql), host)
        assert arr.type == typ and len(arr) == 0 and arr.null_count == 0, (sql, arr.type, len(arr), arr.null_count)
        if typ == pa.bool_():
            kept = chq.filter_record(dev, empty_aliases(host), parse_expr(sql), ctx=ctx).to_host()
            assert kept.num_rows == 0 and kept.schema.names == host.schema.names, (sql, kept.num_rows)


def tiled(table_values, n):
    """n rows cycling through a table, as index array + the table"""
    return np.arange(n) % len(table_values)


@pytest.mark.parametrize("src,dst", [("i32", "i64"), ("i32", "i8"), ("i32", "bool"), ("bool", "i16"), ("i32", "utf8"), ("utf8", "i32"), ("f32", "i32")])
def test_second_round_of_the_capped_grids(ctx, src, dst):
    n = SECOND_ROUND_ROWS
    table = R.clean_rows(src, dst)[:64]
    idx = tiled(table, n)
    # the last row -- alone in the second round -- holds the one failing value, where the pair has one
    failing = R.failing_rows(src, dst)
    tvalid = [True] * len(table)
    want_t, _, _ = R.cast_rows(table, tvalid, src, dst)
    last = failing[0] if failing else table[(n - 1) % len(table)]
    if src == "utf8":
        lens = np.array([len(b) for b in table], np.int64)[idx]
        lens[-1] = len(last)
        offs = np.zeros(n + 1, np.int64)
        np.cumsum(lens, out=offs[1:])
        reps, rem = divmod(n - 1, len(table))
        data = b"".join(table) * reps + b"".join(table[:rem]) + last
        col = pa.Array.from_buffers(pa.utf8(), n, [None, pa.py_buffer(offs.astype(np.int32).tobytes()), pa.py_buffer(data)], null_count=0)
    elif src == "bool":
        bits = np.array(table, bool)[idx]
        bits[-1] = last
        col = pa.Array.from_buffers(pa.bool_(), n, [None, pa.py_buffer(np.packbits(bits, bitorder="little").tobytes())], null_count=0)
    else:
        dtype = F.FORMATS[src].utype if src in R.FLOATS else I.TYPES[src].dtype
        vals = np.array(table, dtype=dtype)[idx]
        vals[-1] = np.array([last], dtype=dtype)[0]
        col = pa.Array.from_buffers(R.ARROW[src], n, [None, pa.py_buffer(vals.tobytes())], null_count=0)
    host = pa.RecordBatch.from_arrays([col], names=["x"])
    dev = chq.DeviceRecordBatch.from_host(host, ctx)
    if failing:
        expect_cast_error(ctx, dev, cast_expr(dst, False), src, dst, host)
    arr = run(ctx, dev, cast_expr(dst, True), host)
    assert len(arr) == n and arr.null_count == (1 if failing else 0)
    if failing:
        assert not arr[n - 1].is_valid and arr[n - 2].is_valid and arr[GRID_ROWS - 1].is_valid
    # the values: the table's reference results, cycled
    if dst == "utf8":
        lens = np.array([len(b) for b in want_t], np.int64)[idx]
        exp_offs = np.zeros(n + 1, np.int64)
        np.cumsum(lens, out=exp_offs[1:])
        assert np.array_equal(np.frombuffer(arr.buffers()[1], np.int32, n + 1), exp_offs)
        reps, rem = divmod(n, len(table))
        assert arr.buffers()[2].to_pybytes()[:int(exp_offs[-1])] == b"".join(want_t) * reps + b"".join(want_t[:rem])
    elif dst == "bool":
        got = np.unpackbits(np.frombuffer(arr.buffers()[1], np.uint8), bitorder="little")[:n].astype(bool)
        assert np.array_equal(got, np.array(want_t, bool)[idx])
    else:
        dtype = F.FORMATS[dst].utype if dst in R.FLOATS else I.TYPES[dst].dtype
        got = np.frombuffer(arr.buffers()[1], dtype, n)
        exp = np.array(want_t, dtype=dtype)[idx]
        stop = n - 1 if failing else n
        assert np.array_equal(got[:stop], exp[:stop])


# ---- sliced views: validity, Boolean values and offsets read from a bit / row offset -------------------------------------------
@pytest.mark.parametrize("off", (1, 7, 63, 65))
def test_sliced_device_views(ctx, off):
    n = 200
    for src, dst in (("bool", "i32"), ("i32", "bool"), ("bool", "utf8"), ("i64", "i16"), ("utf8", "i64"), ("f32", "u8"), ("i16", "utf8"), ("utf8", "bool"), ("bool", "f16")):
        values = cycled(R.bool_strings() if (src, dst) == ("utf8", "bool") else R.edges(src), n + off + 3)
        valid = spread_nulls(len(values), 3, 2)
        host = batch_of(values, valid, src)
        view = chq.DeviceRecordBatch.from_host(host, ctx).slice(off, n)
        want, wvalid, _ = R.cast_rows(values[off:off + n], valid[off:off + n], src, dst)
        check_array(run(ctx, view, cast_expr(dst, True), host), want, wvalid, dst, f"{src}->{dst} view at {off}")
        check_array(run(ctx, host.slice(off, n), cast_expr(dst, True)), want, wvalid, dst, f"{src}->{dst} host slice at {off}")


def test_one_row_batch_next_to_a_literal(ctx):
    host = pa.RecordBatch.from_arrays([pa.array([41], pa.int32()), pa.array(["0041"])], names=["id", "s"])
    for sql, want in (("cast(id as bigint) + 1", pa.array([42], pa.int64())), ("cast(s as int) + 1", pa.array([42], pa.int32())),
                      ("cast(id as varchar) || 'x'", pa.array(["41x"])), ("1 + s::bigint", pa.array([42], pa.int64()))):
        arr, _ = chq.compute_value(host, empty_aliases(host), parse_expr(sql), ctx=ctx)
        assert arr.equals(want), (sql, arr)


# ---- failures count on valid rows only; lazy errors -------------------------------------------------------------------------------
def test_failures_on_valid_rows_only(ctx):
    strings = [b"12", b"abc", b"-7", b"", b"+3", b"99999999999"]
    valid = [True, False, True, False, True, False]
    host = batch_of(strings, valid, "utf8", "s")
    arr = run(ctx, host, cast_expr("i32", False, "s"))
    check_array(arr, [12, 0, -7, 0, 3, 0], valid, "i32", "unparsable strings in null slots")
    ints = [1, 300, -128, -129, 127, 1 << 40]
    host = batch_of(ints, valid, "i64")
    check_array(run(ctx, host, cast_expr("i8", False)), [1, 0, -128, 0, 127, 0], valid, "i8", "out-of-range values in null slots")
    nan = F.FORMATS["f64"].default_nan
    host = batch_of([F.encode(0, 1.5, "f64"), nan, F.encode(1, 2.5, "f64"), F.FORMATS["f64"].inf_bits, 0, F.encode(0, 2**70, "f64")], valid, "f64")
    check_array(run(ctx, host, cast_expr("i32", False)), [1, 0, -2, 0, 0, 0], valid, "i32", "NaN / inf / huge in null slots")
    host = batch_of([b"yes", b"maybe", b"0", b"2", b" F ", b"tru e"], valid, "utf8", "s")
    check_array(run(ctx, host, cast_expr("bool", False, "s")), [True, False, False, False, False, False], valid, "bool", "bad spellings in null slots")
    # ... and the same values in valid slots fail
    expect_cast_error(ctx, batch_of(strings, [True] * 6, "utf8", "s"), cast_expr("i32", False, "s"), "utf8", "i32")
    expect_cast_error(ctx, batch_of(ints, [True] * 6, "i64"), cast_expr("i8", False), "i64", "i8")


def lazy_batch():
    s = ["0x1", "12", "0abc", "7", None, "0", "-3", "00", "+8"]
    return pa.RecordBatch.from_arrays([pa.array(s), pa.array(list(range(len(s))), pa.int32())], names=["s", "id"])


def test_lazy_errors_in_case_and_coalesce(ctx):
    host = lazy_batch()
    s = host.column("s").to_pylist()
    guarded = "case when s like '0%' then 0 else cast(s as int) end"
    arr, _ = chq.compute_value(host, empty_aliases(host), parse_expr(guarded), ctx=ctx)
    want = [None if v is None else 0 if v.startswith("0") else int(v) for v in s]
    assert arr.type == pa.int32() and arr.to_pylist() == want
    # without the guard the same rows fail
    with pytest.raises(chq.ChqError) as ei:
        chq.compute_value(host, empty_aliases(host), parse_expr("cast(s as int)"), ctx=ctx)
    assert ei.value.code == R.CAST_ERROR
    with pytest.raises(chq.ChqError) as ei:      # a guard that lets an unparsable row through
        chq.compute_value(host, empty_aliases(host), parse_expr("case when s like '0a%' then 0 else cast(s as int) end"), ctx=ctx)
    assert ei.value.code == R.CAST_ERROR
    arr, _ = chq.compute_value(host, empty_aliases(host), parse_expr("coalesce(try_cast(s as int), cast('-1' as int))"), ctx=ctx)
    ref = [R.cast_value(v.encode(), "utf8", "i32") if v is not None else R.FAIL for v in s]
    assert arr.null_count == 0 and arr.to_pylist() == [-1 if r is R.FAIL else r for r in ref]
    arr, _ = chq.compute_value(host, empty_aliases(host), parse_expr("try_cast(s as int) is not null"), ctx=ctx)
    assert arr.to_pylist() == [r is not R.FAIL for r in ref]
    # a device view takes the same route
    dev = chq.DeviceRecordBatch.from_host(host, ctx)
    arr, _ = chq.compute_value(dev, empty_aliases(host), parse_expr(guarded), ctx=ctx)
    assert arr.to_pylist() == want


# ---- composition: filter_record, a group (the per-batch route), project_record ------------------------------------------------------
def table(n, seed):
    rng = np.random.default_rng(seed)
    ids = rng.integers(-2**31, 2**31 - 1, n, dtype=np.int64).astype(np.int32)
    edge = [0, -1, 2**31 - 1, -2**31][:n]
    ids[:len(edge)] = edge
    codes = [str(int(v)) for v in rng.integers(0, 250, n)]
    if n > 2:
        codes[1] = "0100"
        codes[2] = "+101"
    value1 = ["v" + str(i % 17) for i in range(n)]
    return pa.RecordBatch.from_arrays([pa.array(ids), pa.array(codes), pa.array(value1), pa.array(rng.random(n).astype(np.float32) * 200 - 100)],
                                      names=["id", "code", "value1", "value2"])


def expected_filter(rec):
    keep = pa.array([int(c) > 100 for c in rec.column("code").to_pylist()])
    return rec.filter(keep)


def test_where_cast_in_filter_record_and_a_group(ctx):
    sel = parse_select("select * from t where cast(code as int) > 100")
    recs = [table(n, seed) for seed, n in enumerate((1000, 1, 2049, 65))]
    for rec in recs:
        for src in (rec, chq.DeviceRecordBatch.from_host(rec, ctx)):
            got = chq.filter_record(src, empty_aliases(rec), sel.selection, ctx=ctx)
            got = got.to_host() if hasattr(got, "to_host") else got
            assert got.equals(expected_filter(rec)), rec.num_rows
    outs = chq.filter_records(recs, empty_aliases(recs[0]), sel.selection, ctx=ctx)
    assert len(outs) == len(recs)
    for rec, got in zip(recs, outs):
        got = got.to_host() if hasattr(got, "to_host") else got
        assert got.equals(expected_filter(rec))
    # a batch of the group with an unparsable code fails the call
    bad = table(50, 9).set_column(1, "code", pa.array(["x"] * 50))
    with pytest.raises(chq.ChqError) as ei:
        chq.filter_records([recs[0], bad], empty_aliases(recs[0]), sel.selection, ctx=ctx)
    assert ei.value.code == R.CAST_ERROR


def test_select_casts_in_project_record(ctx):
    rec = table(3000, 5)
    sel = parse_select("select cast(id as bigint) * 1000000 as wide, cast(id as varchar) || '-' || value1 as tag, cast(value2 as int) v, "
                       "try_cast(code as tinyint) small, id::double as d, upper(cast(id > 0 as varchar)) as pos from t")
    for src in (rec, chq.DeviceRecordBatch.from_host(rec, ctx)):
        got = chq.project_record(sel.projection, src, empty_aliases(rec), ctx=ctx)
        got = got.to_host() if hasattr(got, "to_host") else got
        ids = rec.column("id").to_pylist()
        assert got.schema.names == ["wide", "tag", "v", "small", "d", "pos"]
        assert got.column("wide").equals(pa.array([i * 1000000 for i in ids], pa.int64()))
        assert got.column("tag").equals(pa.array([f"{i}-{v}" for i, v in zip(ids, rec.column("value1").to_pylist())]))
        assert got.column("v").equals(pc.cast(pc.trunc(rec.column("value2")), pa.int32()))
        small = [int(c) if int(c) <= 127 else None for c in rec.column("code").to_pylist()]
        assert got.column("small").equals(pa.array(small, pa.int8())) and got.column("small").null_count > 0
        assert got.column("d").equals(pc.cast(rec.column("id"), pa.float64()))
        assert got.column("pos").equals(pa.array(["TRUE" if i > 0 else "FALSE" for i in ids]))
        # an output column is nullable iff it holds a null
        assert [f.nullable for f in got.schema] == [False, False, False, True, False, False]
    # checked Int32 arithmetic overflows where the cast does not
    with pytest.raises(chq.ChqError) as ei:
        chq.project_record(parse_select("select id * 1000000 from t").projection, rec, empty_aliases(rec), ctx=ctx)
    assert ei.value.code == 20


def test_cast_like_and_comparison(ctx):
    rec = table(500, 3)
    ids = rec.column("id").to_pylist()
    arr, _ = chq.compute_value(rec, empty_aliases(rec), parse_expr("cast(id as varchar) like '1%'"), ctx=ctx)
    assert arr.to_pylist() == [str(i).startswith("1") for i in ids]
    arr, _ = chq.compute_value(rec, empty_aliases(rec), parse_expr("cast(id as varchar) = '-1'"), ctx=ctx)
    assert arr.to_pylist() == [i == -1 for i in ids]
    arr, _ = chq.compute_value(rec, empty_aliases(rec), parse_expr("cast(cast(id as varchar) as int) = id"), ctx=ctx)
    assert arr.to_pylist() == [True] * len(ids)
