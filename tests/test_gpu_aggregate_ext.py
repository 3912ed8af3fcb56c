"""GPU: the GROUP BY items AVG and COUNT(DISTINCT), and HAVING in the aggregate operator, against the host reference of
tests/aggregate_ext_reference.py.

Compared exactly: keys, counts, COUNT(DISTINCT), MIN / MAX, integer sums, the group order, the null placement, and AVG over
integers -- RN(exact total) / count has one correct value.  AVG over floats is checked twice:

  bit for bit   in a call that also holds SUM and COUNT of the same column the AVG bits are np.float64(sum) / np.float64(count)
                of THAT call's sum and count, wherever the sum is finite (a NaN compares as NaN with any payload).  No
                tolerance: the average is the very sum in one IEEE division.
  reference     |got - exp| <= ns * 2^-52 * mags / count + 2^-52 * |exp| per group: the SUM bound of test_gpu_aggregate.compare
                (twice the first-order bound of any summation order in binary64) divided by the count, plus one rounding of
                the division.  Derived, not measured."""
import json
import math

import numpy as np
import pyarrow as pa
import pytest

import chapterhouseqe_amd as chq
from chapterhouseqe_amd import sqlast as A
from chapterhouseqe_amd.sqlparse import aggregate_plan, having_plan, parse_select

from . import aggregate_ext_reference as X
from . import sort_reference as R
from . import test_gpu_sorted_stats as S
from .helpers import arrays_identical, explain_diff
from .test_gpu_aggregate import shapes, value_columns
from .test_gpu_sort import KINDS, key_array, payload_batch, utf8_from_bytes

pytestmark = pytest.mark.gpu

T = 2048   # sorted positions per workgroup tile of the segmented reduce (aggregate_device.h kAggTile)
NEW_KINDS = (A.AggKind.AVG, A.AggKind.COUNT_DISTINCT)


@pytest.fixture(scope="module")
def ctx():
    return chq.Context(0)


def aliases(rec):
    return [[] for _ in range(rec.num_columns)]


def compare(got, exp, bounds, items):
    assert got.num_columns == exp.num_columns and got.num_rows == exp.num_rows, (got.num_rows, exp.num_rows, got.schema, exp.schema)
    for c in range(exp.num_columns):
        fg, fe = got.schema.field(c), exp.schema.field(c)
        assert (fg.name, fg.type, fg.nullable) == (fe.name, fe.type, fe.nullable), (c, fg, fg.nullable, fe, fe.nullable)
        a, e = got.column(c), exp.column(c)
        if c not in bounds:
            assert arrays_identical(a, e), explain_diff(got.select([c]), exp.select([c]))
            continue
        assert a.null_count == e.null_count and a.is_valid().equals(e.is_valid()), fe.name
        ns, mags = bounds[c]
        assert ns.max(initial=0) <= 10**6
        for g, (x, y) in enumerate(zip(a.to_pylist(), e.to_pylist())):
            if y is None:
                continue
            if math.isnan(y) or math.isinf(y):
                assert (math.isnan(x) and math.isnan(y)) or x == y, (fe.name, g, x, y)
            elif items[c][0] == "avg":
                bound = float(ns[g]) * 2.0**-52 * float(mags[g]) / float(ns[g]) + 2.0**-52 * abs(y)
                assert abs(x - y) <= bound, (fe.name, g, x, y, int(ns[g]), float(mags[g]))
            else:
                assert abs(x - y) <= float(ns[g]) * 2.0**-52 * float(mags[g]), (fe.name, g, x, y, int(ns[g]), float(mags[g]))


def check(ctx, rec, keys, items, device_in=False, device_result=None, exp=None):
    k, it = X.to_plan(keys, items)
    src = chq.DeviceRecordBatch.from_host(rec, ctx) if device_in else rec
    got = chq.aggregate_record(src, aliases(rec), k, it, ctx=ctx, device_result=device_result)
    if isinstance(got, chq.DeviceRecordBatch):
        got = got.to_host()
    e, bounds = exp if exp is not None else X.aggregate(rec, keys, items)
    compare(got, e, bounds, items)
    return got


def check_avg_bits(got, avg, total, count):
    """AVG is this call's own SUM over this call's own COUNT in one IEEE division"""
    valid = np.asarray(got.column(avg).is_valid())
    assert valid.tolist() == (np.asarray(got.column(count).to_numpy(zero_copy_only=False)) > 0).tolist()
    s = got.column(total).fill_null(0).to_numpy(zero_copy_only=False).astype(np.float64)[valid]
    c = got.column(count).to_numpy(zero_copy_only=False).astype(np.float64)[valid]
    m = got.column(avg).fill_null(0).to_numpy(zero_copy_only=False).astype(np.float64)[valid]
    with np.errstate(all="ignore"):
        want = s / c
    fin = np.isfinite(s)
    assert m[fin].view(np.uint64).tolist() == want[fin].view(np.uint64).tolist()
    assert np.isnan(m[~fin]).tolist() == np.isnan(s[~fin]).tolist() and (m[~fin][~np.isnan(s[~fin])] == s[~fin][~np.isnan(s[~fin])]).all()
    return int(fin.sum())


# ---- row counts x group shapes ---------------------------------------------------------------------------------------------
NEW_ITEMS = [("key", "k", 0), ("avg", "m_i64", "i64"), ("avg", "m_f64", "f64"), ("sum", "s_f64", "f64"), ("count", "c_f64", "f64"),
             ("avg", "m_f32", "f32"), ("sum", "s_f32", "f32"), ("count", "c_f32", "f32"), ("avg", "m_i16", "i16"), ("avg", "m_u8", "u8"),
             ("count_distinct", "d_i16", "i16"), ("count_distinct", "d_u8", "u8"), ("count_distinct", "d_f32", "f32"),
             ("count_distinct", "d_k", "k"), ("count_star", "n", None)]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 5])
def test_row_counts_and_group_shapes(ctx, n):
    rng = np.random.default_rng(n)
    vals = value_columns(rng, n)
    # few distinct values, so that COUNT(DISTINCT) is neither 1 nor the count
    vals = [(c, pa.array(rng.integers(-4, 4, n).astype(np.int16), mask=rng.random(n) < 0.5) if c == "i16" else
             pa.array(rng.integers(0, 3, n).astype(np.uint8)) if c == "u8" else a) for c, a in vals]
    for nulls in (True, False):
        cols = [a if nulls else pa.array(a.fill_null(1).to_numpy(zero_copy_only=False)) for _, a in vals]
        for name, key in shapes(n).items():
            rec = pa.RecordBatch.from_arrays([pa.array(key.astype(np.int32))] + cols, names=["k"] + [c for c, _ in vals])
            exp = X.aggregate(rec, ["k"], NEW_ITEMS)
            for device_in in (False, True):
                got = check(ctx, rec, ["k"], NEW_ITEMS, device_in=device_in, exp=exp)
                assert got.num_rows == len(np.unique(key)), name
                check_avg_bits(got, "m_f64", "s_f64", "c_f64")
                check_avg_bits(got, "m_f32", "s_f32", "c_f32")
                assert got.column("d_k").to_pylist() == [1] * got.num_rows
    s = ctx.last_stats()
    assert s["rows_in"] == n and s["rows_out"] == got.num_rows and (n == 0 or s["launches"] > 0)


def test_zero_keys_and_zero_rows(ctx):
    rng = np.random.default_rng(1)
    items = [it for it in NEW_ITEMS if it[0] != "key" and it[2] != "k"]
    for n in (0, 1, 5000):
        vals = value_columns(rng, n)
        rec = pa.RecordBatch.from_arrays([a for _, a in vals], names=[c for c, _ in vals])
        for device_in in (False, True):
            got = check(ctx, rec, [], items, device_in=device_in)
            assert got.num_rows == 1 and got.column("n").to_pylist() == [n]
    empty = rec.slice(0, 0)
    got = check(ctx, empty, [], items)
    assert got.to_pylist() == [{name: (0 if kind in ("count", "count_distinct", "count_star") else None) for kind, name, _ in items}]
    assert [f.nullable for f in got.schema] == [kind in ("avg", "sum") for kind, _, _ in items]
    assert check(ctx, empty, ["u8"], [("key", "u8", 0)] + items).num_rows == 0


# ---- AVG ---------------------------------------------------------------------------------------------------------------------
def test_avg_float_edge_values(ctx):
    inf, nan = math.inf, math.nan
    groups = [[1.0, nan, 2.0], [inf, 1.0, -inf], [inf, 5.0, inf], [-inf, -1e300], [None, None, None], [None, 2.5, None], [-0.0, -0.0],
              [5e-324, 5e-324, 5e-324], [1.0, 2.0, 4.0], [5e307, 4e307, -5e307]]
    keys, vals = [], []
    for g, xs in enumerate(groups):
        keys += [g] * len(xs)
        vals += xs
    items = [("key", "k", 0), ("avg", "m", "v"), ("sum", "s", "v"), ("count", "c", "v")]
    for t in (pa.float64(), pa.float32()):
        tv = [None if v is None else (v if t == pa.float64() or math.isinf(v) or math.isnan(v) or 1e-38 < abs(v) < 1e38 or v == 0 else
                                      math.copysign(1e38 if abs(v) > 1 else 2.0**-149, v)) for v in vals]
        rec = pa.RecordBatch.from_arrays([pa.array(keys, type=pa.int32()), pa.array(tv, type=t)], names=["k", "v"])
        got = check(ctx, rec, ["k"], items)
        assert check_avg_bits(got, "m", "s", "c") == 5
        m = got.column(1).to_pylist()
        assert math.isnan(m[0]) and math.isnan(m[1]) and m[2:4] == [inf, -inf] and m[4] is None and m[5] == 2.5
        assert math.copysign(1.0, m[6]) == -1.0 and m[6] == 0.0 and m[8] == 7.0 / 3.0            # -0 / 2 = -0
        if t == pa.float64():
            assert m[7] == 5e-324                                                              # 3 * tiny / 3
    # a group spread over several tiles: the partials meet in the fold, and the average is still that sum over the count
    n = 3 * T + 5
    rng = np.random.default_rng(3)
    rec = pa.RecordBatch.from_arrays([pa.array(np.zeros(n, np.int32)), pa.array(rng.standard_normal(n) * 1e3, mask=rng.random(n) < 0.2)], names=["k", "v"])
    got = check(ctx, rec, ["k"], items)
    assert check_avg_bits(got, "m", "s", "c") == 1


U64MAX, I64MAX, I64MIN = 2**64 - 1, 2**63 - 1, -2**63
RN_GROUPS_U64 = [[U64MAX, 2**11 + 2],                 # 2^64 + 2^11 + 1: sticky in the low word, up
                 [U64MAX, 2**11 + 1],                 # 2^64 + 2^11: a tie whose guard bit is in the low word, to even (2^64)
                 [U64MAX, 3 * 2**11 + 1],             # 2^64 + 3 * 2^11: a tie on an odd mantissa, up
                 [U64MAX, 1], [U64MAX], [0, 0, 0], [2**53, 1], [2**53, 3], [2**53, 2],
                 [U64MAX, U64MAX - 2**12 + 1],        # 2^65 - 2^12: 53 ones, exact
                 [U64MAX, U64MAX - 2**11 + 1],        # 2^65 - 2^11: the tie above it carries out of the mantissa into 2^65
                 [U64MAX, U64MAX - 2**10 + 1],        # 2^65 - 2^10: so does the value above the tie
                 [U64MAX] * 7, [U64MAX, U64MAX, U64MAX, 5]]
RN_GROUPS_I64 = [[I64MAX, I64MAX], [I64MIN, I64MIN], [I64MIN], [I64MAX], [-2**53, -1], [-2**53, -3], [2**53, 1], [I64MAX, I64MIN],
                 [I64MIN, I64MIN, I64MIN, -1], [I64MAX, I64MAX, I64MAX, 1], [-1, 1], [I64MIN + 1, -(2**10) - 1, I64MIN]]


@pytest.mark.parametrize("groups,t", [(RN_GROUPS_U64, pa.uint64()), (RN_GROUPS_I64, pa.int64())])
def test_avg_of_integers_is_the_rounded_exact_total_over_the_count(ctx, groups, t):
    keys = [g for g, xs in enumerate(groups) for _ in xs]
    rec = pa.RecordBatch.from_arrays([pa.array(keys, type=pa.int32()), pa.array([x for xs in groups for x in xs], type=t)], names=["k", "v"])
    items = [("key", "k", 0), ("avg", "m", "v"), ("count", "c", "v")]
    for device_in in (False, True):
        got = check(ctx, rec, ["k"], items, device_in=device_in)
        assert got.column(1).to_pylist() == [float(sum(xs)) / float(len(xs)) for xs in groups]
    if t == pa.int64():
        assert got.column(1).to_pylist()[0] == 9.223372036854775807e18
    # SUM over the same column, in a call of its own, still overflows
    k, it = X.to_plan(["k"], [("key", "k", 0), ("sum", "total", "v")])
    with pytest.raises(chq.ChqError) as ei:
        chq.aggregate_record(rec, aliases(rec), k, it, ctx=ctx)
    assert ei.value.code == 20 and "total" in str(ei.value)


def test_avg_of_integers_over_a_group_of_three_tiles(ctx):
    n = 3 * T + 5
    key = np.zeros(n, np.int32)
    key[-2:] = 1
    rng = np.random.default_rng(8)
    v = np.where(rng.random(n) < 0.7, I64MAX, rng.integers(I64MAX - 2**40, I64MAX, n))
    rec = pa.RecordBatch.from_arrays([pa.array(key), pa.array(v, type=pa.int64(), mask=rng.random(n) < 0.1),
                                      pa.array(np.full(n, U64MAX, np.uint64))], names=["k", "v", "u"])
    got = check(ctx, rec, ["k"], [("key", "k", 0), ("avg", "m", "v"), ("avg", "mu", "u"), ("count", "c", "v")], device_in=True)
    assert got.column(2).to_pylist() == [float((n - 2) * U64MAX) / float(n - 2), float(2 * U64MAX) / 2.0]
    check(ctx, rec, [], [("avg", "m", "v"), ("avg", "mu", "u")])


SUMMABLE = ["int8", "int16", "int32", "int64", "uint8", "uint16", "uint32", "uint64", "float32", "float64"]


@pytest.mark.parametrize("kind", SUMMABLE)
def test_avg_over_every_supported_input_type(ctx, kind):
    rng = np.random.default_rng(SUMMABLE.index(kind))
    n = 2 * T + 77
    vals = key_array(rng, n, kind, True)
    if kind in ("float32", "float64"):      # finite values (the edge values have a test of their own)
        vals = pa.array((rng.standard_normal(n) * rng.choice([1e-3, 1.0, 1e6], n)).astype(np.float32 if kind == "float32" else np.float64),
                        mask=rng.random(n) < 0.15)
    key = np.sort(rng.integers(0, 40, n)).astype(np.int32)
    key[:300] = -1                                    # a group whose values are all null
    valid = np.asarray(vals.is_valid().to_numpy(zero_copy_only=False)).copy()
    valid[:300] = False
    vals = pa.Array.from_buffers(vals.type, n, [pa.array(valid).buffers()[1], vals.buffers()[1]], null_count=int((~valid).sum()))
    rec = pa.RecordBatch.from_arrays([pa.array(key), vals], names=["k", "v"])
    got = check(ctx, rec, ["k"], [("key", "k", 0), ("avg", "m", "v"), ("count", "c", "v"), ("count_distinct", "d", "v")])
    assert got.column(1)[0].as_py() is None and got.column(1).null_count == 1 and got.column(3)[0].as_py() == 0


# ---- COUNT(DISTINCT) -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_count_distinct_over_every_key_type(ctx, kind):
    rng = np.random.default_rng(KINDS.index(kind))
    n = 3000
    rec = pa.RecordBatch.from_arrays([pa.array(rng.integers(0, 6, n).astype(np.int32), mask=rng.random(n) < 0.1), key_array(rng, n, kind, True),
                                      key_array(rng, n, kind, False)], names=["k", "v", "w"])
    items = [("key", "k", 0), ("count_distinct", "d", "v"), ("count", "c", "v"), ("count_distinct", "dw", "w")]
    got = check(ctx, rec, ["k"], items, device_in=KINDS.index(kind) % 2 == 0)
    assert got.num_rows == 7 and all(0 < d <= c for d, c in zip(got.column(1).to_pylist(), got.column(2).to_pylist()))
    check(ctx, rec, [], items[1:])


def test_count_distinct_tells_float_zero_signs_and_nan_payloads_apart(ctx):
    for ut, ft in ((np.uint16, np.float16), (np.uint32, np.float32), (np.uint64, np.float64)):
        bits = 8 * np.dtype(ut).itemsize
        sign, nan = 1 << (bits - 1), ((1 << (bits - 1)) - 1) & ~((1 << {16: 9, 32: 22, 64: 51}[bits]) - 1)   # quiet NaN, payload 0
        pats = np.array([0, sign, nan | 1, nan | 2, nan | 1 | sign, 0, sign, nan | 1, sign, 0, 0, sign, 0], dtype=ut)
        key = np.array([0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 2], np.int32)
        rec = pa.RecordBatch.from_arrays([pa.array(key), pa.array(pats.view(ft))], names=["k", "f"])
        got = check(ctx, rec, ["k"], [("key", "k", 0), ("count_distinct", "d", "f")])
        assert got.column(1).to_pylist() == [5, 2, 1]
        assert check(ctx, rec, [], [("count_distinct", "d", "f")]).column(0).to_pylist() == [5]


def test_count_distinct_over_utf8_values_that_are_prefixes_of_each_other(ctx):
    rng = np.random.default_rng(6)
    base = [b"", b"a", b"ab", b"ab\x00", b"abc", b"abcdefg", b"abcdefgh", b"abcdefghi", b"abcdefgh\x00", b"b", b"\xc3\xa9", b"a" * 40,
            b"a" * 41, b"a" * 40 + b"b"]
    n = 5000
    key = rng.integers(0, 4, n).astype(np.int32)
    pick = np.where(key == 0, rng.integers(0, len(base), n), np.where(key == 1, rng.integers(0, 3, n), rng.integers(5, 9, n)))
    vals = [base[i] for i in pick]
    valid = rng.random(n) < 0.9
    rec = pa.RecordBatch.from_arrays([pa.array(key), utf8_from_bytes(vals, valid)], names=["k", "s"])
    got = check(ctx, rec, ["k"], [("key", "k", 0), ("count_distinct", "d", "s")], device_in=True)
    assert got.column(1).to_pylist() == [len(base), 3, 4, 4]
    assert check(ctx, rec, [], [("count_distinct", "d", "s")]).column(0).to_pylist() == [len(base)]


def test_count_distinct_group_kinds_and_several_items(ctx):
    rng = np.random.default_rng(9)
    sizes = [700, 1, 900, 2500, 3]                     # all null, a single row, one repeated value, all distinct, the null key
    key = np.repeat(np.arange(len(sizes)), sizes).astype(np.int32)
    n = len(key)
    v = np.concatenate([np.zeros(700), [7], np.full(900, -3), np.arange(2500), [1, 1, 2]]).astype(np.int64)
    valid = key != 0
    w = rng.integers(0, 5, n).astype(np.int8)
    order = rng.permutation(n)                         # (the rows arrive unsorted)
    kv = pa.array(key[order], mask=(key == 4)[order])
    rec = pa.RecordBatch.from_arrays([kv, pa.array(v[order], mask=~valid[order]), pa.array(w[order], mask=rng.random(n) < 0.2)], names=["k", "v", "w"])
    items = [("key", "k", 0), ("count_distinct", "d", "v"), ("count_distinct", "again", "v"), ("count_distinct", "dw", "w"),
             ("avg", "m", "v"), ("count_distinct", "dk", "k"), ("count_star", "n", None)]
    got = check(ctx, rec, ["k"], items)
    assert got.column("d").to_pylist() == [0, 1, 1, 2500, 2] == got.column("again").to_pylist()
    assert got.column("dk").to_pylist() == [1, 1, 1, 1, 0]                 # the argument is the key: 1, and 0 for the null group
    one_sort = ctx.last_stats()["launches"]
    check(ctx, rec, [], [it for it in items if it[0] != "key"], device_in=True)
    check(ctx, rec, ["k", "w"], [("key", "k", 0), ("key", "w", 1), ("count_distinct", "d", "v"), ("count_distinct", "dw", "w")])
    # the items over one column share its sort and its run finding: a second item over `v` costs one launch
    check(ctx, rec, ["k"], [it for it in items if it[1] != "again"])
    assert ctx.last_stats()["launches"] == one_sort - 1


def test_fine_runs_and_groups_that_end_around_a_tile_boundary(ctx):
    n = 3 * T + 5
    pos = np.arange(n, dtype=np.int64)
    for cut in (T - 1, T, T + 1):
        for key in ((pos >= cut).astype(np.int32), np.zeros(n, np.int32), (pos // (cut // 2)).astype(np.int32)):
            # sorted by (key, v): fine runs end at cut too, and at 2 * cut; the tail of every group is null
            v = (pos >= cut).astype(np.int64) + (pos >= 2 * cut) + pos // 1000
            rec = pa.RecordBatch.from_arrays([pa.array(key), pa.array(v, mask=(pos % cut) >= cut - 3),
                                              pa.array(pos.astype(np.int32))], names=["k", "v", "row"])
            check(ctx, rec, ["k"], [("key", "k", 0), ("count_distinct", "d", "v"), ("count_distinct", "dr", "row"), ("avg", "m", "v")],
                  device_in=cut == T)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
PAYLOAD_ITEMS = [("key", "k", 0), ("avg", "m_u8", "u8"), ("avg", "m_f", "f64"), ("sum", "s_f", "f64"), ("count", "c_f", "f64"),
                 ("count_distinct", "ds", "s"), ("count_distinct", "db", "b"), ("count_distinct", "ddec", "dec"),
                 ("count_distinct", "df16", "f16"), ("count_distinct", "dts", "ts"), ("count_distinct", "du8", "u8")]


@pytest.mark.parametrize("offset,length", [(1, 5000), (7, 3000), (64, 100), (4097, 2500), (13, 0)])
def test_sliced_device_views(ctx, offset, length):
    rng = np.random.default_rng(offset)
    parent = payload_batch(rng, 7000)
    dev = chq.DeviceRecordBatch.from_host(parent, ctx).slice(offset, length)
    view = parent.slice(offset, length)
    k, it = X.to_plan(["k"], PAYLOAD_ITEMS)
    got = chq.aggregate_record(dev, aliases(parent), k, it, ctx=ctx).to_host()
    compare(got, *X.aggregate(view, ["k"], PAYLOAD_ITEMS), PAYLOAD_ITEMS)
    check_avg_bits(got, "m_f", "s_f", "c_f")
    for keys in (["b", "s"], ["u8"]):        # Boolean and Utf8 keys, and a key with nulls, read at the view's offset
        items = [("key", f"k{j}", j) for j in range(len(keys))] + PAYLOAD_ITEMS[1:]
        k, it = X.to_plan(keys, items)
        got = chq.aggregate_record(dev, aliases(parent), k, it, ctx=ctx).to_host()
        compare(got, *X.aggregate(view, keys, items), items)
    check(ctx, view, ["k"], PAYLOAD_ITEMS, device_result=True)        # a sliced host view


def test_group_of_batches_some_of_them_empty(ctx):
    rng = np.random.default_rng(4)
    batches = []
    for b in range(60):
        n = 0 if b % 7 == 3 else int(rng.integers(1, 400))
        batches.append(pa.RecordBatch.from_arrays([pa.array(rng.integers(0, 50, n).astype(np.int32), mask=rng.random(n) < 0.05),
                                                   pa.array(["%02d" % v for v in rng.integers(0, 20, n)], type=pa.utf8()),
                                                   pa.array((rng.random(n) * 100).astype(np.float32), mask=rng.random(n) < 0.1),
                                                   pa.array(np.arange(n, dtype=np.int64) + 1000 * b)], names=["k", "s", "value2", "id"]))
    items = [("key", "k", 0), ("avg", "m", "value2"), ("avg", "mid", "id"), ("count_distinct", "ds", "s"), ("count_distinct", "dv", "value2")]
    k, it = X.to_plan(["k"], items)
    exp = X.aggregate_batches(batches, ["k"], items)
    compare(chq.aggregate_records(batches, aliases(batches[0]), k, it, ctx=ctx), *exp, items)
    dev = [chq.DeviceRecordBatch.from_host(b, ctx) for b in batches]
    got = chq.aggregate_records(dev, aliases(batches[0]), k, it, ctx=ctx)
    assert isinstance(got, chq.DeviceRecordBatch) and got.num_rows == 51
    compare(got.to_host(), *exp, items)
    compare(chq.aggregate_records(chq.RecordGroup(dev, ctx), aliases(batches[0]), k, it, ctx=ctx, device_result=False), *exp, items)


# ---- errors --------------------------------------------------------------------------------------------------------------------------
FORMATS = {"f16": "e", "b": "b", "ts": "tsm:", "dec": "d:20,2", "s": "u", "fsb4": "w:4", "fsb16": "w:16"}


def test_errors_leave_no_output(ctx):
    rec = payload_batch(np.random.default_rng(3), 100)
    al = aliases(rec)

    def fails(keys, items, code, *mentions):
        for src in (rec, chq.DeviceRecordBatch.from_host(rec, ctx)):
            with pytest.raises(chq.ChqError) as ei:
                chq.aggregate_record(src, al, keys, items, ctx=ctx)      # nothing comes back
            assert ei.value.code == code, (keys, items, ei.value)
            for m in mentions:
                assert m in str(ei.value), ei.value

    key = [A.ident("k")]
    for col in ("f16", "b", "ts", "dec", "s", "fsb4"):
        fails(key, [A.AggItem(A.AggKind.AVG, "x", -1, A.ident(col))], 30, "AVG", f"'{col}'", f"'{FORMATS[col]}'")
    for col in ("fsb16", "fsb4"):
        fails(key, [A.AggItem(A.AggKind.COUNT_DISTINCT, "x", -1, A.ident(col))], 30, f"'{col}'", f"'{FORMATS[col]}'")
        fails([], [A.AggItem(A.AggKind.COUNT_STAR, "n"), A.AggItem(A.AggKind.COUNT_DISTINCT, "x", -1, A.ident(col))], 30, f"'{col}'")
    fails(key, [A.AggItem(8, "x", -1, A.ident("u8"))], 22, "unknown aggregate kind 8")
    fails(key, [A.AggItem(-1, "x", -1, A.ident("u8"))], 22, "unknown aggregate kind")
    plus = A.binop(A.ident("k"), A.BinaryOperator.Plus, A.number("1"))
    for kind in NEW_KINDS:
        fails(key, [A.AggItem(kind, "x", -1, A.ident("nope"))], 7)                             # the evaluator's statuses
        fails(key, [A.AggItem(kind, "x", -1, plus)], 30)                                       # an expression as the argument
        fails(key, [A.AggItem(kind, "x", -1, A.Nested(A.ident("u8")))], 30)
    # aliases resolve like compute_value's
    ta = [["t"] for _ in range(rec.num_columns)]
    got = chq.aggregate_record(rec, ta, [A.compound("t", "k")], [A.AggItem(A.AggKind.KEY, "k", 0), A.AggItem(A.AggKind.AVG, "m", -1, A.compound("t", "u8")),
                                                                  A.AggItem(A.AggKind.COUNT_DISTINCT, "d", -1, A.compound("t", "s"))], ctx=ctx)
    items = [("key", "k", 0), ("avg", "m", "u8"), ("count_distinct", "d", "s")]
    compare(got, *X.aggregate(rec, ["k"], items), items)


# ---- the front-end and the operator ----------------------------------------------------------------------------------------------------
def test_the_sql_front_end_builds_the_same_calls(ctx):
    rng = np.random.default_rng(2)
    n = 4000
    rec = pa.RecordBatch.from_arrays([pa.array(rng.integers(0, 9, n).astype(np.int8), mask=rng.random(n) < 0.1),
                                      pa.array(["ab"[i] for i in rng.integers(0, 2, n)]), pa.array(rng.random(n))], names=["a", "b", "v"])
    keys, plan = aggregate_plan(parse_select("select avg(v), b, avg(a) as mean from t group by a, b"))
    got = chq.aggregate_record(rec, aliases(rec), keys, plan, ctx=ctx)
    rk, ri = X.from_plan(keys, plan)
    compare(got, *X.aggregate(rec, rk, ri), ri)
    assert got.schema.names == ["avg(v)", "b", "mean"] and got.num_rows == 20
    keys, plan = aggregate_plan(parse_select("select distinct b, a as x from t"))
    got = chq.aggregate_record(rec, aliases(rec), keys, plan, ctx=ctx, device_result=True).to_host()
    rk, ri = X.from_plan(keys, plan)
    compare(got, *X.aggregate(rec, rk, ri), ri)
    assert got.schema.names == ["b", "x"] and got.num_rows == 20
    rows = [(r["b"], r["x"]) for r in got.to_pylist()]
    assert rows == sorted(set(rows), key=lambda r: (r[0], r[1] is None, r[1]))           # every pair once, in key order


def test_aggregate_operator_with_having_end_to_end_on_the_device():
    from chapterhouseqe_amd.operators import (AggregateOperatorTask, ExchangeOperator, FilterOperatorTask, OperatorInstanceConfig,
                                              build_default_operator_task_registry)
    from chapterhouseqe_amd.sample_data import simple_batches
    from oracle import oracle as O
    batches = simple_batches(20_000, 2, 500)
    sel = parse_select("select value1, avg(id) as m, min(id), count(*) from t where id > 100 group by value1 "
                       "having count(*) > 1 and max(value2) > 50 and value1 < 'p'")
    keys, items, predicate, n_visible = having_plan(sel)
    assert n_visible == 4 and [(i.kind, i.name) for i in items[4:]] == [(A.AggKind.MAX, "__having_0")]
    exs = [ExchangeOperator(f"operator_p{i}_exchange", [f"operator_p{i + 1}_producer"]) for i in range(3)]
    for rid, b in enumerate(batches):
        exs[0].send_record(rid, b, aliases(b))
    exs[0].producers_completed()
    reg = build_default_operator_task_registry("/tmp")
    ftask = FilterOperatorTask(sel.selection)
    assert reg.find_task_builder(ftask).build(OperatorInstanceConfig(1, "operator_p1_producer", 7, ftask), [exs[0]], exs[1])() is None
    exs[1].producers_completed()
    atask = AggregateOperatorTask(keys, items, 16, predicate, n_visible)
    arun = reg.find_task_builder(atask).build(OperatorInstanceConfig(2, "operator_p2_producer", 7, atask), [exs[1]], exs[2])
    assert arun() is None
    exs[2].producers_completed()
    got = []
    while True:
        r = exs[2].get_next_record("operator_p3_producer", 1)
        if not isinstance(r, tuple):
            break
        got.append(r)
        exs[2].operator_completed_record_processing("operator_p3_producer", r[0])
    assert [r[0] for r in got] == list(range(len(got))) and arun.task.records_sent == len(got) and exs[1].num_records() == 0
    filtered = [O.filter_record(b, aliases(b), sel.selection) for b in batches]
    rk, ri = X.from_plan(keys, items)
    full, _ = X.aggregate_batches(filtered, rk, ri)
    exp = X.having(full, lambda r: r["count(*)"] > 1 and r["__having_0"] > 50 and r["value1"] < "p").select(list(range(n_visible)))
    # a pass-through projection gives a column without a null as not nullable (the evaluator's rule)
    exp = pa.RecordBatch.from_arrays(exp.columns, schema=pa.schema([pa.field(f.name, f.type, exp.column(i).null_count > 0)
                                                                    for i, f in enumerate(exp.schema)]))
    assert 16 < exp.num_rows < full.num_rows and len(got) == -(-exp.num_rows // 16) and arun.task.rows_out == exp.num_rows
    assert all(len(r[2]) == n_visible for r in got)
    parts = [r[1].to_host() if isinstance(r[1], chq.DeviceRecordBatch) else r[1] for r in got]
    compare(R.join(parts), exp, {}, ri)


def test_visible_items_that_share_a_name_keep_their_own_columns_on_the_device():
    from chapterhouseqe_amd.operators import (AggregateOperatorTask, ExchangeOperator, OperatorInstanceConfig,
                                              build_default_operator_task_registry)
    from chapterhouseqe_amd.sample_data import simple_batches
    batches = simple_batches(5000, 2, 500)
    sel = parse_select("select count(*) as x, min(id) as x, max(value2) from t having max(id) > 0")
    keys, items, predicate, n_visible = having_plan(sel)
    assert n_visible == 3 and [i.name for i in items] == ["x", "x", "max(value2)", "__having_0"]
    exs = [ExchangeOperator(f"operator_p{i}_exchange", [f"operator_p{i + 1}_producer"]) for i in range(2)]
    for rid, b in enumerate(batches):
        exs[0].send_record(rid, b, aliases(b))
    exs[0].producers_completed()
    atask = AggregateOperatorTask(keys, items, 16, predicate, n_visible)
    reg = build_default_operator_task_registry("/tmp")
    assert reg.find_task_builder(atask).build(OperatorInstanceConfig(1, "operator_p1_producer", 7, atask), [exs[0]], exs[1])() is None
    exs[1].producers_completed()
    got = exs[1].get_next_record("operator_p2_producer", 1)[1]
    got = got.to_host() if isinstance(got, chq.DeviceRecordBatch) else got
    ids = [v for b in batches for v in b.column(0).to_pylist()]
    v2 = [v for b in batches for v in b.column(2).to_pylist()]
    assert got.schema.names == ["x", "x", "max(value2)"]
    assert [got.column(i).to_pylist() for i in range(3)] == [[len(ids)], [min(ids)], [max(v2)]]


# ---- the existing items ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [T, 3 * T + 5])
def test_a_call_without_the_new_kinds_launches_what_it_launched_before(ctx, n):
    """The figures come from the golden statistics of the sorted operators, recorded before AVG and COUNT(DISTINCT) existed.
    The calls measured are therefore the ones that file pins -- `test_gpu_sorted_stats.AGG_ITEMS` over its fixed batch, every
    aggregate kind that existed -- and not the `ITEMS` list of `test_gpu_aggregate`, for which no recorded figure exists and
    none is made up here."""
    with open(S.GOLDEN) as f:
        golden = json.load(f)
    rec = S.batch(n)
    old = [A.AggItem(A.AggKind.KEY, "k1", key_index=0)] + S.AGG_ITEMS
    chq.aggregate_record(rec, S.aliases(rec), S.ids(["k1"]), old, ctx=ctx)
    before = ctx.last_stats()
    assert {k: int(before[k]) for k in S.KEYS} == golden[f"n{n}/agg/by_k1/host"]
    chq.aggregate_record(rec, S.aliases(rec), [], S.AGG_ITEMS, ctx=ctx)
    assert int(ctx.last_stats()["launches"]) == golden[f"n{n}/agg/no_key/host"]["launches"]
    # an AVG item is one reduce more (and a fold past one tile) and the validity pack; nothing else moves
    chq.aggregate_record(rec, S.aliases(rec), S.ids(["k1"]), old + [A.AggItem(A.AggKind.AVG, "m", column=A.ident("f"))], ctx=ctx)
    assert int(ctx.last_stats()["launches"]) == golden[f"n{n}/agg/by_k1/host"]["launches"] + (2 if n > T else 1) + 1
