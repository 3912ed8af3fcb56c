"""GPU: ORDER BY (chq_sort_record / chq_sort_records) compared exactly -- NaN payloads included -- with the host reference
of tests/sort_reference.py: every key type in both directions and both null placements, tile-edge row counts, float and
integer extremes, Utf8 prefixes, multi-key ties, every payload type, sliced device views, host / device inputs and
outputs, limits, groups, errors, a 2^28-row run checked on the device, and the operator pipeline end to end."""
import decimal
import os
import threading

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

import chapterhouseqe_amd as chq
from chapterhouseqe_amd import sqlast as A
from chapterhouseqe_amd.sqlparse import parse_select

from . import sort_reference as R
from . import typed_reference as TR
from .helpers import batches_identical, explain_diff

pytestmark = pytest.mark.gpu

TILE = 2048   # pairs per workgroup tile of a radix pass (sort_device.h kSortTile)


@pytest.fixture(scope="module")
def ctx():
    return chq.Context(0)


def _split_fsb(rec):
    """(FixedSizeBinary columns, the others): tests.helpers compares every other type; these are compared here"""
    fsb = [i for i, f in enumerate(rec.schema) if pa.types.is_fixed_size_binary(f.type)]
    return fsb, [i for i in range(rec.num_columns) if i not in fsb]


def identical(got, exp):
    fsb, rest = _split_fsb(exp)
    if got.num_columns != exp.num_columns:
        return False
    for i in fsb:
        a, b = got.column(i), exp.column(i)
        if got.schema.field(i) != exp.schema.field(i) or a.null_count != b.null_count or a.to_pylist() != b.to_pylist():
            return False
    return batches_identical(got.select(rest), exp.select(rest))


def explain(got, exp):
    rest = _split_fsb(exp)[1]
    return explain_diff(got.select(rest), exp.select(rest)) if got.num_columns == exp.num_columns else "column counts differ"


def ob(keys):
    return [A.OrderByExpr(A.ident(n), not d, nf) for n, d, nf in keys]


def aliases(rec):
    return [[] for _ in range(rec.num_columns)]


def check(ctx, rec, keys, limit=None, device_in=False, device_result=None, exp_source=None):
    src = chq.DeviceRecordBatch.from_host(rec, ctx) if device_in else rec
    got = chq.sort_record(src, aliases(rec), ob(keys), limit=limit, ctx=ctx, device_result=device_result)
    if isinstance(got, chq.DeviceRecordBatch):
        got = got.to_host()
    exp = R.sort_batch(exp_source if exp_source is not None else rec, keys, limit)
    assert identical(got, exp), explain(got, exp)
    return got


# ---- key columns ----------------------------------------------------------------------------------------------------------
def float_bits(rng, n, width):
    ut = {2: np.uint16, 4: np.uint32, 8: np.uint64}[width]
    ft = {2: np.float16, 4: np.float32, 8: np.float64}[width]
    vals = rng.choice(np.array([0, -0.0, 1.5, -1.5, np.inf, -np.inf, 3.25, -2.0], dtype=ft), n).view(ut).copy()
    bits = 8 * width
    exp_mask = ((1 << (bits - 1)) - 1) & ~((1 << {2: 10, 4: 23, 8: 52}[width]) - 1)
    special = rng.random(n)
    payload = rng.integers(1, 1 << {2: 9, 4: 22, 8: 51}[width], n).astype(ut)
    nan = (ut(exp_mask) | payload) | np.where(rng.random(n) < 0.5, ut(1 << (bits - 1)), ut(0)).astype(ut)
    sub = rng.integers(1, 1 << 8, n).astype(ut) | np.where(rng.random(n) < 0.5, ut(1 << (bits - 1)), ut(0)).astype(ut)
    vals = np.where(special < 0.15, nan, np.where(special < 0.25, sub, vals))
    return pa.array(vals.view(ft))


def key_array(rng, n, kind, nulls):
    mask = (rng.random(n) < 0.15) if nulls else None
    small = rng.integers(-3, 3, n)
    if kind in ("int8", "int16", "int32", "int64"):
        t = getattr(np, kind)
        info = np.iinfo(t)
        v = np.where(rng.random(n) < 0.5, small, rng.integers(info.min, info.max, n, dtype=t, endpoint=True)).astype(t)
        v[: min(n, 2)] = [info.min, info.max][: min(n, 2)]
        return pa.array(v, mask=mask)
    if kind in ("uint8", "uint16", "uint32", "uint64"):
        t = getattr(np, kind)
        info = np.iinfo(t)
        v = np.where(rng.random(n) < 0.5, small & 3, rng.integers(0, info.max, n, dtype=t, endpoint=True)).astype(t)
        return pa.array(v, mask=mask)
    if kind in ("float16", "float32", "float64"):
        arr = float_bits(rng, n, {"float16": 2, "float32": 4, "float64": 8}[kind])
        return pa.Array.from_buffers(arr.type, n, [pa.array(~mask).buffers()[1] if mask is not None else None, arr.buffers()[1]],
                                     null_count=int(mask.sum()) if mask is not None else 0)
    if kind == "bool":
        return pa.array(rng.random(n) < 0.5, mask=mask)
    if kind == "decimal":
        vals = [decimal.Decimal(int(x) * 10 ** int(e)).scaleb(-4) for x, e in zip(rng.integers(-10**9, 10**9, n), rng.integers(0, 20, n))]
        return pa.array(vals, type=pa.decimal128(38, 4), mask=mask)
    if kind in ("decimal32", "decimal64"):   # keys of up to 8 bytes: ordered as their signed integers
        t, it = (pa.decimal32(9, 2), np.int32) if kind == "decimal32" else (pa.decimal64(18, 4), np.int64)
        info = np.iinfo(it)
        v = np.where(rng.random(n) < 0.5, small, rng.integers(info.min, info.max, n, dtype=it, endpoint=True)).astype(it)
        v[: min(n, 3)] = [info.min, info.max, -1][: min(n, 3)]
        return TR.decimal_array(v.tolist(), None if mask is None else ~mask, t)
    if kind == "decimal128_edges":           # raw patterns: every byte of the key takes values other than 0x00 / 0xFF
        edges = TR.I128_EDGES
        return TR.decimal128_array([edges[i] for i in rng.integers(0, len(edges), n)], None if mask is None else ~mask)
    if kind == "utf8":
        pool = ["", "a", "ab", "ab\x00", "abc", "b", "é", "zz", "a" * 7, "a" * 8, "a" * 9, "a" * 8 + "b"]
        return pa.array([pool[i] for i in rng.integers(0, len(pool), n)], mask=mask)
    raw = rng.integers(-(1 << 40), 1 << 40, n).astype(np.int64)
    raw = np.where(rng.random(n) < 0.3, small, raw)
    types = {"date32": pa.date32(), "date64": pa.date64(), "time32s": pa.time32("s"), "time32ms": pa.time32("ms"),
             "time64us": pa.time64("us"), "time64ns": pa.time64("ns"), "ts_us_utc": pa.timestamp("us", tz="UTC"),
             "ts_ns": pa.timestamp("ns"), "duration_ms": pa.duration("ms")}
    t = types[kind]
    if t.bit_width == 32:
        raw = (raw % (1 << 20)).astype(np.int32) - (1 << 19)
        if kind == "time32s":
            raw = np.abs(raw) % 86400
        elif kind == "time32ms":
            raw = np.abs(raw) % 86_400_000
    elif kind in ("time64us", "time64ns"):
        raw = np.abs(raw) % 86_400_000_000
    elif kind == "date64":
        raw = (raw % 200_000 - 100_000) * 86_400_000
    return pa.array(raw, mask=mask).view(t) if mask is None else pa.Array.from_buffers(
        t, n, [pa.array(~mask).buffers()[1], pa.array(raw).buffers()[1]], null_count=int(mask.sum()))


KINDS = ["int8", "int16", "int32", "int64", "uint8", "uint16", "uint32", "uint64", "float16", "float32", "float64", "bool",
         "date32", "date64", "time32s", "time32ms", "time64us", "time64ns", "ts_us_utc", "ts_ns", "duration_ms", "decimal", "utf8",
         "decimal32", "decimal64", "decimal128_edges"]


def keyed_batch(rng, n, kind, nulls=True):
    return pa.RecordBatch.from_arrays([key_array(rng, n, kind, nulls), pa.array(np.arange(n, dtype=np.int32))], names=["k", "row"])


@pytest.mark.parametrize("kind", KINDS)
def test_every_key_type_both_directions_and_null_placements(ctx, kind):
    rng = np.random.default_rng(KINDS.index(kind))
    rec = keyed_batch(rng, 5000, kind)
    for desc in (False, True):
        for nulls_first in (False, True):
            check(ctx, rec, [("k", desc, nulls_first)])


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 10**6, (1 << 24) + 3])
def test_row_counts(ctx, n):
    rng = np.random.default_rng(n % 997)
    rec = pa.RecordBatch.from_arrays([pa.array(rng.integers(-1000, 1000, n).astype(np.int32)),
                                      pa.array(rng.random(n).astype(np.float32), mask=rng.random(n) < 0.1),
                                      pa.array(np.arange(n, dtype=np.int64))], names=["i", "f", "row"])
    check(ctx, rec, [("i", False, False)], device_in=True)
    if n <= 10**6:
        check(ctx, rec, [("f", True, True), ("i", False, False)])


def test_constant_and_all_null_keys_skip_every_pass(ctx):
    n = 10_000
    rec = pa.RecordBatch.from_arrays([pa.array(np.full(n, 7, np.int64)), pa.array([None] * n, type=pa.float32()),
                                      pa.array(np.arange(n, dtype=np.int32))], names=["c", "z", "row"])
    for keys in ([("c", False, False)], [("z", True, True)], [("c", True, False), ("z", False, True)]):
        got = check(ctx, rec, keys)
        assert got.column(2).to_pylist() == list(range(n))
    s = ctx.last_stats()
    assert s["rows_in"] == n and s["rows_out"] == n and s["launches"] > 0


def test_small_int_keys_with_constant_high_bytes(ctx):
    rng = np.random.default_rng(5)
    n = 300_000
    rec = pa.RecordBatch.from_arrays([pa.array(rng.integers(0, 200, n).astype(np.int64)), pa.array(np.arange(n, dtype=np.int32))],
                                     names=["k", "row"])
    check(ctx, rec, [("k", False, False)])
    small = ctx.last_stats()["launches"]
    rec2 = pa.RecordBatch.from_arrays([pa.array(rng.integers(-2**62, 2**62, n).astype(np.int64)), pa.array(np.arange(n, dtype=np.int32))],
                                      names=["k", "row"])
    check(ctx, rec2, [("k", False, False)])
    assert ctx.last_stats()["launches"] > small    # one digit pass against eight


def utf8_from_bytes(vals, valid=None):
    offs = np.zeros(len(vals) + 1, np.int32)
    np.cumsum([len(v) for v in vals], out=offs[1:])
    bitmap = None if valid is None else pa.py_buffer(np.packbits(valid, bitorder="little").tobytes())
    return pa.Array.from_buffers(pa.utf8(), len(vals), [bitmap, pa.py_buffer(offs.tobytes()), pa.py_buffer(b"".join(vals))],
                                 null_count=0 if valid is None else int((~valid).sum()))


def test_utf8_keys_prefixes_nuls_and_non_ascii(ctx):
    rng = np.random.default_rng(9)
    base = []
    for plen in (0, 7, 8, 9, 64, 300):
        p = bytes(rng.integers(97, 100, plen).astype(np.uint8))
        base += [p, p + b"\x00", p + b"a", p + b"b", p + b"\xc3\xa9", p + b"\x00\x00", p + b"a\x00", p + b"ab"]
    base += [b"", b"", b"\x00", b"\x7f", b"\xe2\x82\xac", b"\xf0\x9f\x98\x80"]
    vals = [base[i] for i in rng.integers(0, len(base), 20_000)]
    valid = rng.random(len(vals)) < 0.9
    rec = pa.RecordBatch.from_arrays([utf8_from_bytes(vals, valid), pa.array(np.arange(len(vals), dtype=np.int32))], names=["s", "row"])
    for desc in (False, True):
        for nf in (False, True):
            check(ctx, rec, [("s", desc, nf)], device_in=desc)


def test_multi_key_ties_are_stable(ctx):
    rng = np.random.default_rng(21)
    n = 50_000
    rec = pa.RecordBatch.from_arrays([
        pa.array([["x", "y", "xy", ""][i] for i in rng.integers(0, 4, n)], mask=rng.random(n) < 0.1),
        pa.array(rng.integers(0, 3, n).astype(np.int32), mask=rng.random(n) < 0.1),
        pa.array(rng.choice([0.0, -0.0, np.nan, 1.0], n).astype(np.float64), mask=rng.random(n) < 0.1),
        pa.array(np.arange(n, dtype=np.int32))], names=["s", "i", "f", "row"])
    for keys in ([("s", False, False), ("i", True, True)], [("i", False, True), ("s", True, False)],
                 [("f", True, False), ("s", False, True), ("i", True, True)], [("i", False, False)]):
        check(ctx, rec, keys)


def payload_batch(rng, n):
    mask = lambda: rng.random(n) < 0.2   # noqa: E731
    return pa.RecordBatch.from_arrays([
        pa.array(rng.integers(0, 50, n).astype(np.int16)),
        pa.array(["p%d" % (i % 37) * (i % 5) for i in range(n)], mask=mask()),
        pa.array(rng.random(n) < 0.5, mask=mask()),
        pa.array(rng.random(n) < 0.5),
        pa.array([decimal.Decimal(int(x)).scaleb(-2) for x in rng.integers(-10**12, 10**12, n)], type=pa.decimal128(20, 2), mask=mask()),
        pa.array(rng.integers(0, 255, n).astype(np.uint8), mask=mask()),
        pa.array(rng.random(n), mask=mask()),
        pa.array(rng.random(n).astype(np.float16)),
        pa.array(rng.integers(0, 1 << 40, n), type=pa.int64()).view(pa.timestamp("ms")),
        pa.array([bytes([i % 251] * 16) for i in range(n)], type=pa.binary(16)),
        pa.array([bytes([i % 7] * 4) for i in range(n)], type=pa.binary(4)),
        pa.array(np.arange(n, dtype=np.int32))],
        names=["k", "s", "b", "b2", "dec", "u8", "f64", "f16", "ts", "fsb16", "fsb4", "row"])


def test_payload_of_every_importable_type(ctx):
    rng = np.random.default_rng(33)
    rec = payload_batch(rng, 7000)
    check(ctx, rec, [("k", False, False)])
    check(ctx, rec, [("k", True, True)], device_in=True, device_result=False)
    check(ctx, rec, [("dec", True, False), ("b", False, True)], device_in=True, device_result=True)


def test_fixed_size_binary_key_is_not_supported(ctx):
    rec = payload_batch(np.random.default_rng(1), 100)
    with pytest.raises(chq.ChqError) as ei:
        chq.sort_record(rec, aliases(rec), ob([("fsb16", False, False)]), ctx=ctx)
    assert ei.value.code == 30


@pytest.mark.parametrize("offset,length", [(1, 5000), (7, 3000), (9, 2049), (64, 100), (4097, 1500), (13, 0)])
def test_sliced_device_views(ctx, offset, length):
    rng = np.random.default_rng(offset)
    parent = payload_batch(rng, 7000)
    dev = chq.DeviceRecordBatch.from_host(parent, ctx).slice(offset, length)
    for keys in ([("s", False, True), ("k", True, False)], [("b", True, False), ("u8", False, True)]):
        got = chq.sort_record(dev, aliases(parent), ob(keys), ctx=ctx).to_host()
        exp = R.sort_batch(parent.slice(offset, length), keys)
        assert identical(got, exp), explain(got, exp)
    host_view = parent.slice(offset, length)
    check(ctx, host_view, [("f64", True, True)], device_result=True)


@pytest.mark.parametrize("limit", [0, 1, 100, 4999, 5000, 10**9])
def test_limit(ctx, limit):
    rng = np.random.default_rng(2)
    rec = payload_batch(rng, 5000)
    got = check(ctx, rec, [("k", False, False), ("s", True, True)], limit=limit)
    assert got.num_rows == min(limit, 5000) and got.schema == rec.schema
    s = ctx.last_stats()
    assert s["rows_in"] == 5000 and s["rows_out"] == min(limit, 5000)


def test_group_of_1000_batches(ctx):
    rng = np.random.default_rng(4)
    batches = []
    for b in range(1000):
        n = 10_000
        batches.append(pa.RecordBatch.from_arrays([pa.array(np.arange(b * n, (b + 1) * n, dtype=np.int32)),
                                                   pa.array(rng.integers(0, 1000, n).astype(np.int32)),
                                                   pa.array((rng.random(n) * 100).astype(np.float32))], names=["id", "k", "value2"]))
    for keys, limit in (([("k", True, False)], None), ([("value2", False, False)], 1000)):
        got = chq.sort_records(batches, aliases(batches[0]), ob(keys), limit=limit, ctx=ctx)
        exp = R.sort_batches(batches, keys, limit)
        assert identical(got, exp), explain(got, exp)
    dev = [chq.DeviceRecordBatch.from_host(b, ctx) for b in batches[:200]]
    got = chq.sort_records(dev, aliases(batches[0]), ob([("k", False, False), ("id", True, False)]), ctx=ctx).to_host()
    exp = R.sort_batches(batches[:200], [("k", False, False), ("id", True, False)])
    assert identical(got, exp), explain(got, exp)


def test_groups_with_empty_batches_mixed_views_and_record_group(ctx):
    rng = np.random.default_rng(8)
    parent = payload_batch(rng, 9000)
    windows = [(0, 0), (3, 1000), (1009, 1), (2000, 0), (2050, 2049), (4097, 3000), (8999, 1)]
    dev_parent = chq.DeviceRecordBatch.from_host(parent, ctx)
    views = [dev_parent.slice(o, n) for o, n in windows]
    host = [parent.slice(o, n) for o, n in windows]
    keys = [("s", True, False), ("k", False, True)]
    got = chq.sort_records(views, aliases(parent), ob(keys), ctx=ctx, device_result=False)
    exp = R.sort_batches(host, keys)
    assert identical(got, exp), explain(got, exp)
    grp = chq.RecordGroup(views, ctx)
    got = chq.sort_records(grp, aliases(parent), ob(keys), limit=77, ctx=ctx).to_host()
    assert identical(got, R.sort_batches(host, keys, 77))
    hgrp = chq.RecordGroup(host, ctx)
    got = chq.sort_records(hgrp, aliases(parent), ob([("dec", False, False)]), ctx=ctx, device_result=True).to_host()
    assert identical(got, R.sort_batches(host, [("dec", False, False)]))
    hgrp.release()


def test_errors_leave_no_output(ctx):
    rec = payload_batch(np.random.default_rng(3), 100)
    al = aliases(rec)
    cases = [([A.OrderByExpr(A.ident("nope"))], 7),
             ([A.OrderByExpr(A.compound("t", "k"))], 8),
             ([A.OrderByExpr(A.binop(A.ident("k"), A.BinaryOperator.Plus, A.number("1")))], 30),
             ([A.OrderByExpr(A.Nested(A.ident("k")))], 30)]
    for order_by, code in cases:
        with pytest.raises(chq.ChqError) as ei:
            chq.sort_record(rec, al, order_by, ctx=ctx)
        assert ei.value.code == code, (order_by, ei.value)
    iv = pa.RecordBatch.from_arrays([pa.array([pa.MonthDayNano([1, 2, 3])] * 3, type=pa.month_day_nano_interval())], names=["iv"])
    with pytest.raises(chq.ChqError) as ei:
        chq.sort_record(iv, [[]], ob([("iv", False, False)]), ctx=ctx)
    assert ei.value.code == 30
    other = pa.RecordBatch.from_arrays([pa.array([1, 2], type=pa.int64())], names=["k"])
    with pytest.raises(chq.ChqError) as ei:
        chq.sort_records([rec, other], al, ob([("k", False, False)]), ctx=ctx)
    assert ei.value.code == 22
    # aliases resolve like compute_value's: t.k with an alias list naming t
    ta = [["t"] for _ in range(rec.num_columns)]
    got = chq.sort_record(rec, ta, [A.OrderByExpr(A.compound("t", "k"))], ctx=ctx)
    assert identical(got, R.sort_batch(rec, [("k", False, False)]))


def test_scale_2_28_rows_checked_on_the_device(ctx):
    import torch
    n = 1 << 28
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1)
    keys = torch.randint(-(1 << 31), (1 << 31) - 1, (n,), dtype=torch.int32, device=dev, generator=g)
    keys[: n // 4] = keys[: n // 4] % 1000       # heavy ties
    rows = torch.arange(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    rec = chq.DeviceRecordBatch.from_device_pointers([("k", "i", keys.data_ptr()), ("row", "i", rows.data_ptr())], n, ctx=ctx)
    out = chq.sort_record(rec, [[], []], ob([("k", False, False)]), ctx=ctx)
    assert out.num_rows == n
    k = out.column_tensor(0, torch)
    r = out.column_tensor(1, torch)
    assert bool((k[1:] >= k[:-1]).all())
    same = k[1:] == k[:-1]
    assert bool((r[1:][same] > r[:-1][same]).all())
    counts = torch.bincount(r.long(), minlength=n)
    assert int(counts.min()) == 1 and int(counts.max()) == 1
    del k, r, counts, same
    out.release()
    rec.release()


def test_order_by_operator_end_to_end(tmp_path):
    from chapterhouseqe_amd.operators import (ExchangeOperator, FilterOperatorTask, FilterTaskBuilder, MaterializeFilesOperatorTask,
                                              MaterializeFilesTaskBuilder, OperatorInstanceConfig, OperatorTaskRegistry,
                                              OrderByOperatorTask, OrderByTaskBuilder)
    from chapterhouseqe_amd.operators.tasks import ReadFilesOperatorTask, ReadFilesTaskBuilder
    from oracle import oracle as O
    rng = np.random.default_rng(12)
    root = tmp_path / "store"
    (root / "data").mkdir(parents=True)
    tables = []
    for k, n in enumerate([25_000, 7, 12_345]):
        t = pa.table({"id": pa.array(np.arange(n, dtype=np.int32) + 100_000 * k),
                      "value1": pa.array(["%03x" % v for v in rng.integers(0, 4096, n)]),
                      "value2": pa.array((rng.random(n) * 100).astype(np.float32), mask=rng.random(n) < 0.05)})
        pq.write_table(t, root / "data" / f"part{k}.parquet", row_group_size=10_000)
        tables.append(t)
    sql = "select id, value1, value2 from read_files('data/*.parquet') where value2 > 10.0 order by value1 desc, value2 limit 20000"
    sel = parse_select(sql)
    exs = [ExchangeOperator(f"operator_p{i}_exchange", [f"operator_p{i + 1}_producer"]) for i in range(3)]
    out_root = tmp_path / "results"
    reg = (OperatorTaskRegistry()
           .add_table_func_task_builder("read_files", ReadFilesTaskBuilder(str(root)))
           .add_filter_task_builder(FilterTaskBuilder(group_size=16))
           .add_order_by_task_builder(OrderByTaskBuilder())
           .add_materialize_files_builder(MaterializeFilesTaskBuilder(str(out_root)), ["parquet"]))
    rtask = ReadFilesOperatorTask("data/*.parquet", alias=None, max_rows_per_batch=4_000)
    assert reg.find_task_builder(rtask).build(OperatorInstanceConfig(1, "operator_p0_producer", 7, rtask), [], exs[0])() is None
    exs[0].producers_completed()
    ftask = FilterOperatorTask(sel.selection)
    assert reg.find_task_builder(ftask).build(OperatorInstanceConfig(2, "operator_p1_producer", 7, ftask), [exs[0]], exs[1])() is None
    exs[1].producers_completed()
    otask = OrderByOperatorTask(sel.order_by, sel.limit, 4096)
    orun = reg.find_task_builder(otask).build(OperatorInstanceConfig(3, "operator_p2_producer", 7, otask), [exs[1]], exs[2])
    err = [None]
    th = threading.Thread(target=lambda: err.__setitem__(0, orun()))
    th.start(); th.join()
    assert err[0] is None and orun.task.records_sent == 5
    exs[2].producers_completed()
    mtask = MaterializeFilesOperatorTask("parquet", sel.projection)
    mrun = reg.find_task_builder(mtask).build(OperatorInstanceConfig(4, "operator_p3_producer", 7, mtask), [exs[2]], None)
    assert mrun() is None
    d = os.path.dirname(mrun.task.files_written[0])
    got = pa.concat_tables([pq.read_table(os.path.join(d, f"rec_{rid}.parquet")) for rid in range(5)])
    whole = pa.concat_tables(tables).combine_chunks().to_batches()[0]
    al = aliases(whole)
    filtered = O.filter_record(whole, al, sel.selection)
    exp = O.project_record(sel.projection, R.sort_batch(filtered, R.keys_of(sel.order_by, filtered.schema), sel.limit), al)
    assert got.to_pydict() == pa.Table.from_batches([exp]).to_pydict()
