"""GPU: hash partitioning (chq_partition_records) compared exactly, partition by partition -- row order, NaN payloads and null
counts included -- with the host reference of tests/partition_reference.py (itself pinned by tests/test_partition_host.py),
and end to end: a join and an aggregate run partition by partition give what the whole gives."""
import numpy as np
import pyarrow as pa
import pytest

import chapterhouseqe_amd as chq
from chapterhouseqe_amd import sqlast as A

from . import join_reference as J
from . import partition_reference as P
from . import sort_reference as R
from .test_gpu_join import aliases, same, to_host
from .test_gpu_sort import KINDS, float_bits, key_array, payload_batch, utf8_from_bytes

pytestmark = pytest.mark.gpu

T = 2048   # rows per workgroup tile (partition_device.h kPartTile)
SIZES = [0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 5]
PARTS = [1, 2, 3, 8, 255, 256]


@pytest.fixture(scope="module")
def ctx():
    return chq.Context(0)


def check(ctx, batches, keys, n_parts, device_in=False, device_result=None):
    """one partitioning of host batches against the reference; returns the parts (on the host)"""
    batches = [batches] if isinstance(batches, pa.RecordBatch) else list(batches)
    src = [chq.DeviceRecordBatch.from_host(b, ctx) for b in batches] if device_in else batches
    got = chq.partition_records(src, aliases(batches[0]), P.to_plan(keys), n_parts, ctx=ctx, device_result=device_result)
    assert isinstance(got, list) and len(got) == n_parts
    dev = device_in if device_result is None else device_result
    assert all(isinstance(g, chq.DeviceRecordBatch) == dev for g in got)
    got = [to_host(g) for g in got]
    exp = P.partition(batches, keys, n_parts)
    for p in range(n_parts):
        same(got[p], exp[p])
    return got


def keyed(keys, name="k"):
    return pa.RecordBatch.from_arrays([keys, pa.array(np.arange(len(keys), dtype=np.int32))], names=[name, "row"])


# ---- row counts x partition counts ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_row_counts_and_partition_counts(ctx, n):
    rng = np.random.default_rng(n)
    rec = keyed(pa.array(rng.integers(0, max(1, n // 3), n).astype(np.int32), mask=rng.random(n) < 0.15))
    for n_parts in PARTS:
        got = check(ctx, rec, ["k"], n_parts, device_in=(n + n_parts) % 2 == 1)
        s = ctx.last_stats()
        assert s["rows_in"] == n and s["rows_out"] == n and sum(g.num_rows for g in got) == n
        assert all(g.schema == rec.schema for g in got)                       # empty partitions keep the full schema
        if n >= T and 1 < n_parts <= 8:
            assert all(g.num_rows > 0 for g in got)                           # (no case passes vacuously)


# ---- key types -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_every_key_type(ctx, kind):
    rng = np.random.default_rng(200 + KINDS.index(kind))
    rec = keyed(key_array(rng, 2500, kind, True))
    got = check(ctx, rec, ["k"], 8, device_in=kind in ("float32", "utf8", "decimal", "bool"))
    assert sum(1 for g in got if g.num_rows) > 1
    check(ctx, rec, ["k"], 3)


@pytest.mark.parametrize("width", [2, 4, 8])
def test_float_keys_are_taken_by_bits(ctx, width):
    rng = np.random.default_rng(width)
    check(ctx, keyed(float_bits(rng, T + 300, width)), ["k"], 8)              # -0, +0 and NaN payloads among the keys
    check(ctx, keyed(float_bits(rng, 500, width)), ["k"], 256, device_in=True)


def test_boolean_key_on_an_odd_bit_offset(ctx):
    rng = np.random.default_rng(5)
    rec = keyed(pa.array(rng.random(3000) < 0.5, mask=rng.random(3000) < 0.15))
    check(ctx, rec, ["k"], 2)
    view = chq.DeviceRecordBatch.from_host(rec, ctx).slice(13, 2500)
    got = chq.partition_records(view, aliases(rec), P.to_plan(["k"]), 3, ctx=ctx)
    for g, e in zip(got, P.partition(rec.slice(13, 2500), ["k"], 3)):
        same(g.to_host(), e)


def test_utf8_keys_of_every_chunk_shape(ctx):
    rng = np.random.default_rng(9)
    base = []
    for length in (0, 1, 7, 8, 9, 16, 17, 40):
        base += [bytes(rng.integers(97, 100, length).astype(np.uint8)) for _ in range(4)]
    base += [b"\x00", b"\x00\x00", b"a\x00", b"\xe2\x82\xac"]          # zero bytes differ from the zero padding by the length

    def batch(n):
        vals = [base[i] for i in rng.integers(0, len(base), n)]
        return keyed(utf8_from_bytes(vals, rng.random(n) < 0.85))          # "" and null both occur

    got = check(ctx, batch(3000), ["k"], 8)
    assert all(g.num_rows for g in got)
    check(ctx, batch(T + 1), ["k"], 255, device_in=True)


# ---- key counts ------------------------------------------------------------------------------------------------------------------
def test_two_keys_of_mixed_types_in_both_orders(ctx):
    rng = np.random.default_rng(21)
    n = 3000
    rec = pa.RecordBatch.from_arrays([
        pa.array([["x", "y", "xy", ""][i] for i in rng.integers(0, 4, n)], mask=rng.random(n) < 0.1),
        pa.array(rng.choice([0.0, -0.0, np.nan, 1.0], n).astype(np.float64), mask=rng.random(n) < 0.1),
        pa.array(np.arange(n, dtype=np.int32))], names=["s", "f", "row"])
    a = check(ctx, rec, ["s", "f"], 8)
    b = check(ctx, rec, ["f", "s"], 8, device_in=True)
    assert [g.num_rows for g in a] != [g.num_rows for g in b]                 # the order of the keys is part of the hash


def test_nine_keys_take_two_hash_launches(ctx):
    rng = np.random.default_rng(22)
    n = T + 700
    cols = [pa.array(rng.integers(0, 2, n).astype(np.int8), mask=(rng.random(n) < 0.1) if i in (0, 8) else None) for i in range(9)]
    rec = pa.RecordBatch.from_arrays(cols + [pa.array(np.arange(n, dtype=np.int32))], names=[f"k{i}" for i in range(9)] + ["row"])
    names = [f"k{i}" for i in range(9)]
    nine = check(ctx, rec, names, 8)
    eight = check(ctx, rec, names[:8], 8, device_in=True)
    assert [g.num_rows for g in nine] != [g.num_rows for g in eight]          # the ninth key and its nulls count
    check(ctx, rec, names + names, 3)                                          # 18 keys: three launches


def test_a_constant_key_puts_every_row_into_one_partition(ctx):
    n = 3 * T + 5
    got = check(ctx, keyed(pa.array(np.full(n, 1, np.int32))), ["k"], 8, device_in=True)
    assert [g.num_rows for g in got] == [n if p == 4 else 0 for p in range(8)]          # Int32 1 -> partition 4 (pinned)
    assert got[4].column(1).to_pylist() == list(range(n))                               # in input order across the tiles
    got = check(ctx, keyed(pa.array([None] * n, type=pa.int32())), ["k"], 8)
    assert got[1].num_rows == n                                                          # null -> partition 1 (pinned)


# ---- payloads and inputs ---------------------------------------------------------------------------------------------------------
def test_payload_of_every_importable_type_and_device_result_both_ways(ctx):
    rng = np.random.default_rng(33)
    rec = payload_batch(rng, 5000)
    check(ctx, rec, ["k"], 8)
    check(ctx, rec, ["k", "b2"], 3, device_in=True, device_result=False)
    check(ctx, rec, ["u8"], 8, device_in=False, device_result=True)
    check(ctx, rec, ["dec", "s"], 256, device_in=True, device_result=True)


@pytest.mark.parametrize("offset,length", [(1, 3000), (9, 2049), (64, 100), (13, 0)])
def test_sliced_views_with_odd_bit_offsets(ctx, offset, length):
    rng = np.random.default_rng(offset)
    rec = payload_batch(rng, 4000)
    view = chq.DeviceRecordBatch.from_host(rec, ctx).slice(offset, length)
    for keys in (["k"], ["s", "b"]):
        got = chq.partition_records(view, aliases(rec), P.to_plan(keys), 8, ctx=ctx)
        for g, e in zip(got, P.partition(rec.slice(offset, length), keys, 8)):
            same(g.to_host(), e)
    check(ctx, rec.slice(offset, length), ["b", "u8"], 3)                      # a sliced host batch


def test_groups_of_batches_with_empty_batches_and_mixed_residency(ctx):
    rng = np.random.default_rng(8)
    rec = payload_batch(rng, 5000)
    cuts = np.sort(rng.integers(0, 5000, 11)).tolist()
    cuts[4] = cuts[3]          # an empty batch
    windows = list(zip([0] + cuts, cuts + [5000]))
    host = [rec.slice(a, b - a) for a, b in windows]
    assert any(b.num_rows == 0 for b in host)
    check(ctx, host, ["k", "b2"], 8)
    check(ctx, host, ["s"], 8, device_in=True)
    dev = chq.DeviceRecordBatch.from_host(rec, ctx)
    mixed = [dev.slice(a, b - a) if i % 3 else host[i] for i, (a, b) in enumerate(windows)]
    exp = P.partition(host, ["k"], 8)
    got = chq.partition_records(mixed, aliases(rec), P.to_plan(["k"]), 8, ctx=ctx)
    assert all(isinstance(g, pa.RecordBatch) for g in got)          # not every input on the device: host results
    for g, e in zip(got, exp):
        same(g, e)
    grp = chq.RecordGroup([dev.slice(a, b - a) for a, b in windows], ctx)
    for _ in range(2):                                               # groups are reusable
        got = chq.partition_records(grp, aliases(rec), P.to_plan(["k"]), 8, ctx=ctx)
        for g, e in zip(got, exp):
            same(g.to_host(), e)


def test_two_calls_give_bit_identical_results(ctx):
    rng = np.random.default_rng(41)
    rec = payload_batch(rng, 3 * T + 5)
    keys = P.to_plan(["k", "b2"])
    a = chq.partition_records(rec, aliases(rec), keys, 8, ctx=ctx)
    b = chq.partition_records(rec, aliases(rec), keys, 8, ctx=ctx)
    assert sum(1 for g in a if g.num_rows) > 1
    for x, y in zip(a, b):
        same(x, y)


def test_stats(ctx):
    rng = np.random.default_rng(42)
    n = 3 * T + 5
    rec = keyed(pa.array(rng.integers(0, 100, n).astype(np.int32), mask=rng.random(n) < 0.15))
    check(ctx, rec, ["k"], 8)
    s = ctx.last_stats()
    assert s["rows_in"] == n and s["rows_out"] == n and s["tiles"] == 4
    assert s["launches"] >= 3 + 3          # hash, scan, scatter + one gather per buffer
    # at least: the keys read once, an id and a row id written per row, and both columns through the permutation
    assert s["bytes_read_alg"] >= n * (4 + 1 + 8) and s["bytes_written_alg"] >= n * (1 + 4 + 8)
    assert s["bytes_read_alg"] < n * 100 and s["bytes_written_alg"] < n * 100
    check(ctx, rec, ["k"], 1)              # one partition: no hash, the columns still move once
    s = ctx.last_stats()
    assert s["rows_out"] == n and s["bytes_written_alg"] >= n * 8


# ---- errors ------------------------------------------------------------------------------------------------------------------------
def test_errors_leave_no_output(ctx):
    rec = payload_batch(np.random.default_rng(3), 100)
    al = aliases(rec)
    k = A.ident("k")
    plus = A.binop(A.ident("k"), A.BinaryOperator.Plus, A.number("1"))
    cases = [([], 8, 22, ""),                                        # no key
             ([k], 0, 22, "n_partitions"), ([k], 257, 22, "n_partitions"), ([k], -1, 22, "n_partitions"),
             ([plus], 8, 30, ""), ([A.Nested(k)], 8, 30, ""),        # an expression as a key
             ([A.ident("fsb16")], 8, 30, "fsb16"), ([k, A.ident("fsb4")], 8, 30, "fsb4"),
             ([A.ident("nope")], 8, 7, ""), ([A.compound("t", "k")], 8, 8, "")]
    for keys, n_parts, code, word in cases:
        for src in (rec, chq.DeviceRecordBatch.from_host(rec, ctx)):
            with pytest.raises(chq.ChqError) as ei:
                chq.partition_records(src, al, keys, n_parts, ctx=ctx)
            assert ei.value.code == code and word in str(ei.value), (keys, n_parts, ei.value)
    with pytest.raises(chq.ChqError) as ei:
        chq.partition_records(rec, al, [A.ident("fsb16")], 8, ctx=ctx)
    assert "'fsb16'" in str(ei.value) and "'w:16'" in str(ei.value)          # the column and its Arrow type
    # aliases resolve like compute_value's
    got = chq.partition_records(rec, [["t"]] * rec.num_columns, [A.compound("t", "k")], 8, ctx=ctx)
    for g, e in zip(got, P.partition(rec, ["k"], 8)):
        same(g, e)


# ---- end to end: a keyed operator run partition by partition -------------------------------------------------------------------------
def rows_of(batches):
    rows = []
    for b in batches:
        rows += list(zip(*[c.to_pylist() for c in b.columns]))
    return sorted(rows, key=repr)


def test_join_partition_by_partition_is_the_whole_join(ctx):
    rng = np.random.default_rng(50)

    def side(n, row_name):
        return pa.RecordBatch.from_arrays([pa.array(rng.integers(0, 100, n).astype(np.int32), mask=rng.random(n) < 0.15),
                                           pa.array(np.arange(n, dtype=np.int32))], names=["k", row_name])

    left, right = side(5000, "lrow"), side(3000, "rrow")
    la, ra = aliases(left), aliases(right)
    lparts = chq.partition_records(chq.DeviceRecordBatch.from_host(left, ctx), la, P.to_plan(["k"]), 8, ctx=ctx)
    rparts = chq.partition_records(right, ra, P.to_plan(["k"]), 8, ctx=ctx, device_result=True)
    pieces = []
    for lp, rp in zip(lparts, rparts):
        got = chq.join_records(lp, la, rp, ra, J.to_plan([("k", "k")]), ctx=ctx).to_host()
        same(got, J.join(lp.to_host(), rp.to_host(), [("k", "k")])[2])
        pieces.append(got)
    whole = J.join(left, right, [("k", "k")])[2]
    assert whole.num_rows > 100_000 and sum(1 for g in pieces if g.num_rows) == 8
    assert rows_of(pieces) == rows_of([whole])


def test_aggregate_partition_by_partition_is_the_whole_aggregate(ctx):
    rng = np.random.default_rng(51)
    n = 5000
    rec = pa.RecordBatch.from_arrays([pa.array(rng.integers(0, 100, n).astype(np.int32), mask=rng.random(n) < 0.15),
                                      pa.array(rng.integers(-1000, 1000, n).astype(np.int64), mask=rng.random(n) < 0.2)], names=["k", "v"])
    al = aliases(rec)
    keys = [A.ident("k")]
    items = [A.AggItem(A.AggKind.KEY, "k", 0), A.AggItem(A.AggKind.COUNT_STAR, "n"), A.AggItem(A.AggKind.COUNT, "c", -1, A.ident("v")),
             A.AggItem(A.AggKind.SUM, "s", -1, A.ident("v")), A.AggItem(A.AggKind.MIN, "lo", -1, A.ident("v")),
             A.AggItem(A.AggKind.MAX, "hi", -1, A.ident("v"))]
    whole = chq.aggregate_records([rec], al, keys, items, ctx=ctx)
    parts = chq.partition_records(rec, al, keys, 8, ctx=ctx, device_result=True)
    pieces = [to_host(chq.aggregate_records([p], al, keys, items, ctx=ctx)) for p in parts]
    assert whole.num_rows == 101 and sum(g.num_rows for g in pieces) == 101          # a group lies wholly inside one partition
    same(R.sort_batch(R.join(pieces), [("k", False, False)]), whole)
