"""GPU: window functions (chq_window_record / chq_window_records) against the host reference of tests/window_reference.py.

Everything is compared bit for bit -- the pass-through columns, ranks, counts, LAG / LEAD, integer sums, MIN, MAX and every
null count -- except a finite float SUM, which is compared with the correctly rounded exact sum of the row's frame:
|got - exact| <= m * 2^-52 * sum|x_i|, m the values in the frame.  That is twice the first-order bound m * 2^-53 * sum|x_i|
of ANY summation order in binary64 (valid while m * 2^-53 < 0.01: no frame here has more than 10^6 rows), the bound of
tests/test_gpu_aggregate.py.  Float sums must also be bit-identical from one call to the next."""
import decimal
import math

import numpy as np
import pyarrow as pa
import pytest

import chapterhouseqe_amd as chq
from chapterhouseqe_amd import sqlast as A
from chapterhouseqe_amd.sqlparse import parse_select, window_plan

from . import sort_reference as R
from . import window_reference as W
from .aggregate_reference import SumOverflow
from .helpers import arrays_identical, explain_diff
from .test_gpu_aggregate import shapes, value_columns
from .test_gpu_sort import KINDS, key_array, payload_batch, utf8_from_bytes

pytestmark = pytest.mark.gpu

T = 2048   # sorted positions per workgroup tile (window_device.h kWinTile)
B = 256    # tiles one round of win_carry_kernel covers (window_device.h kWinCarryRound)


@pytest.fixture(scope="module")
def ctx():
    return chq.Context(0)


def aliases(rec):
    return [[] for _ in range(rec.num_columns)]


def compare(got, exp, bounds):
    assert got.num_columns == exp.num_columns and got.num_rows == exp.num_rows, (got.num_rows, exp.num_rows, got.schema, exp.schema)
    for c in range(exp.num_columns):
        fg, fe = got.schema.field(c), exp.schema.field(c)
        assert (fg.name, fg.type, fg.nullable) == (fe.name, fe.type, fe.nullable), (c, fg, fg.nullable, fe, fe.nullable)
        a, e = got.column(c), exp.column(c)
        if pa.types.is_fixed_size_binary(fe.type):     # (tests.helpers compares every other type)
            assert a.null_count == e.null_count and a.to_pylist() == e.to_pylist(), fe.name
            continue
        if c not in bounds:
            assert a.null_count == e.null_count, (fe.name, a.null_count, e.null_count)
            assert arrays_identical(a, e), (fe.name, explain_diff(got.select([c]), exp.select([c])))
            continue
        assert a.null_count == e.null_count and a.is_valid().equals(e.is_valid()), fe.name
        ns, mags = bounds[c]
        assert ns.max(initial=0) <= 10**6
        for r, (x, y) in enumerate(zip(a.to_pylist(), e.to_pylist())):
            if y is None:
                continue
            if math.isnan(y) or math.isinf(y):
                assert (math.isnan(x) and math.isnan(y)) or x == y, (fe.name, r, x, y)
            else:
                assert abs(x - y) <= float(ns[r]) * 2.0**-52 * float(mags[r]), (fe.name, r, x, y, int(ns[r]), float(mags[r]))


def check(ctx, rec, partition_by, order_by, items, device_in=False, device_result=None, exp=None):
    p, o, it = W.to_plan(partition_by, order_by, items)
    src = chq.DeviceRecordBatch.from_host(rec, ctx) if device_in else rec
    got = chq.window_record(src, aliases(rec), p, o, it, ctx=ctx, device_result=device_result)
    if isinstance(got, chq.DeviceRecordBatch):
        got = got.to_host()
    e, bounds = exp if exp is not None else W.window(rec, partition_by, order_by, items)
    compare(got, e, bounds)
    return got


def bits(col):
    return col.to_numpy(zero_copy_only=False).view(np.uint64).tolist()


# ---- row counts x partition shapes x peer shapes -------------------------------------------------------------------------------
def all_items():
    """all ten kinds, the aggregates in all three frames"""
    items = [("row_number", "rn", None, "partition", 0), ("rank", "rk", None, "partition", 0), ("dense_rank", "dr", None, "partition", 0),
             ("lag", "lag_f32", "f32", "partition", 1), ("lead", "lead_i16", "i16", "partition", 3)]
    for f in W.FRAMES:
        items += [("count_star", f"n_{f}", None, f, 0), ("count", f"c_{f}", "i16", f, 0), ("sum", f"si_{f}", "i64", f, 0),
                  ("sum", f"sf_{f}", "f64", f, 0), ("min", f"lo_{f}", "f32", f, 0), ("max", f"hi_{f}", "i16", f, 0)]
    return items


def peer_shapes(n):
    """sorted Int32 order keys (non-decreasing in sorted position): where the peer groups begin"""
    pos = np.arange(n, dtype=np.int64)
    straddle = pos.copy()
    straddle[max(0, T - 5):T + 5] = max(0, T - 5)
    return {"all peers": np.zeros(n, np.int64), "no peers": pos, "peers of 3": pos // 3, "a peer group straddles a tile boundary": straddle}


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 5])
def test_row_counts_partition_shapes_and_peer_shapes(ctx, n):
    rng = np.random.default_rng(n)
    vals = value_columns(rng, n)
    shuffle = rng.permutation(n)                       # the rows arrive in no order: the sort has to find the shapes
    items = all_items()
    for pname, part in shapes(n).items():
        for qname, peer in peer_shapes(n).items():
            rec = pa.RecordBatch.from_arrays([pa.array(part[shuffle].astype(np.int32)), pa.array(peer[shuffle].astype(np.int32))] + [a for _, a in vals],
                                             names=["p", "o"] + [c for c, _ in vals])
            got = check(ctx, rec, ["p"], [("o", False, False)], items, device_in=n % 2 == 1)
            assert got.num_rows == n, (pname, qname)
    s = ctx.last_stats()
    assert s["rows_in"] == n and s["rows_out"] == n and (n == 0 or s["launches"] > 0)
    assert n == 0 or (s["bytes_read_alg"] > 0 and s["bytes_written_alg"] > 0)


def test_a_partition_over_more_tiles_than_one_carry_round(ctx):
    rng = np.random.default_rng(8)
    n = (B + 1) * T + 5
    tail = 300                                         # a second, short partition behind the long one
    rec = pa.RecordBatch.from_arrays([pa.array((np.arange(n) >= n - tail).astype(np.int8)),
                                      pa.array(rng.integers(-128, 128, n).astype(np.int8), mask=rng.random(n) < 0.1),
                                      pa.array(rng.integers(0, 1000, n).astype(np.float32))], names=["p", "v", "w"])
    items = [("sum", "sv", "v", "rows", 0), ("sum", "sw", "w", "rows", 0), ("max", "hi", "v", "rows", 0), ("count", "c", "v", "partition", 0)]
    got = check(ctx, rec, ["p"], [], items, device_in=True)
    # Float32 integers below 2^24 whose totals stay below 2^53: every running sum is exact
    exp = np.concatenate([np.cumsum(rec.column(2).to_numpy()[:n - tail].astype(np.float64)), np.cumsum(rec.column(2).to_numpy()[n - tail:].astype(np.float64))])
    assert got.column(4).to_numpy().tolist() == exp.tolist()


# ---- keys ----------------------------------------------------------------------------------------------------------------------
KEY_ITEMS = [("row_number", "rn", None, "partition", 0), ("rank", "rk", None, "partition", 0), ("dense_rank", "dr", None, "partition", 0),
             ("count_star", "n", None, "range", 0), ("sum", "s", "v", "rows", 0), ("lag", "prev", "row", "partition", 1)]


@pytest.mark.parametrize("nulls", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_every_key_type_as_partition_key_and_as_order_key(ctx, kind, nulls):
    rng = np.random.default_rng(KINDS.index(kind) + 100 * nulls)
    n = 3000
    rec = pa.RecordBatch.from_arrays([key_array(rng, n, kind, nulls), pa.array(np.arange(n, dtype=np.int32)),
                                      pa.array(rng.integers(0, 4, n).astype(np.int8)),
                                      pa.array(rng.integers(-100, 100, n).astype(np.int64), mask=rng.random(n) < 0.3)], names=["k", "row", "g", "v"])
    check(ctx, rec, ["k"], [("v", False, False)], KEY_ITEMS)
    check(ctx, rec, ["g"], [("k", True, True)], KEY_ITEMS, device_in=True)           # DESC, NULLS FIRST
    check(ctx, rec, [], [("k", False, True), ("g", True, False)], KEY_ITEMS)


def test_more_keys_than_one_heads_launch_compares(ctx):
    rng = np.random.default_rng(21)
    n = 6000
    rec = pa.RecordBatch.from_arrays([
        pa.array([["x", "y", "xy", ""][i] for i in rng.integers(0, 4, n)], mask=rng.random(n) < 0.1),
        pa.array(rng.integers(0, 3, n).astype(np.int32), mask=rng.random(n) < 0.1),
        pa.array(rng.choice([0.0, -0.0, np.nan, 1.0], n).astype(np.float64), mask=rng.random(n) < 0.1),
        pa.array(rng.random(n) < 0.5), pa.array(rng.integers(0, 2, n).astype(np.uint8)),
        pa.array(rng.integers(0, 3, n).astype(np.int16)), pa.array(rng.integers(0, 3, n).astype(np.int64), mask=rng.random(n) < 0.2),
        pa.array(rng.random(n)), pa.array(np.arange(n, dtype=np.int32))], names=["s", "i", "f", "b", "u", "h", "l", "v", "row"])
    part = ["s", "i", "f", "b", "u"]
    order = [("h", True, False), ("l", False, True), ("s", True, True), ("i", False, False)]
    items = KEY_ITEMS[:4] + [("sum", "sv", "v", "range", 0), ("max", "last", "row", "rows", 0)]
    check(ctx, rec, part, order, items)
    check(ctx, rec, part[:2], order[:1], items, device_in=True)


def test_float_zero_signs_and_nan_payloads_are_partitions_and_peers_of_their_own(ctx):
    for ut, ft in ((np.uint16, np.float16), (np.uint32, np.float32), (np.uint64, np.float64)):
        nb = 8 * np.dtype(ut).itemsize
        sign, nan = 1 << (nb - 1), ((1 << (nb - 1)) - 1) & ~((1 << {16: 9, 32: 22, 64: 51}[nb]) - 1)   # quiet NaN, payload 0
        pats = np.array([0, sign, nan | 1, nan | 2, nan | 1 | sign, 0, sign, nan | 1, sign], dtype=ut)
        rec = pa.RecordBatch.from_arrays([pa.array(pats.view(ft)), pa.array(np.arange(len(pats), dtype=np.int32))], names=["f", "row"])
        got = check(ctx, rec, ["f"], [], [("count_star", "n", None, "partition", 0), ("row_number", "rn", None, "partition", 0)])
        assert got.column(2).to_pylist() == [2, 3, 2, 1, 1, 2, 3, 2, 3] and got.column(3).to_pylist() == [1, 1, 1, 1, 1, 2, 2, 2, 3]
        got = check(ctx, rec, [], [("f", False, False)], [("dense_rank", "dr", None, "partition", 0), ("count_star", "n", None, "range", 0)])
        # totalOrder: -NaN < -0 < +0 < +NaN(1) < +NaN(2)
        assert got.column(2).to_pylist() == [3, 2, 4, 5, 1, 3, 2, 4, 2] and got.column(3).to_pylist() == [6, 4, 8, 9, 1, 6, 4, 8, 4]


# ---- LAG / LEAD ------------------------------------------------------------------------------------------------------------------
def test_lag_and_lead_of_every_column_type(ctx):
    rng = np.random.default_rng(12)
    n = 2 * T + 100
    mask = lambda: rng.random(n) < 0.2   # noqa: E731
    words = [b"", b"a", b"lorem ipsum dolor sit amet, consectetur adipiscing elit", b"\xc3\xa9", b"x" * 33, b"ab"]
    part = np.where(np.arange(n) < T + 700, 0, 1 + (np.arange(n) - (T + 700)) // 40)          # one partition longer than T + 1 rows
    shuffle = rng.permutation(n)
    rec = pa.RecordBatch.from_arrays([
        pa.array(part[shuffle].astype(np.int32)), pa.array(rng.random(n)),
        pa.array(rng.integers(-128, 128, n).astype(np.int8), mask=mask()),
        pa.array(rng.integers(-2**62, 2**62, n), type=pa.int64(), mask=mask()),
        pa.array(rng.standard_normal(n).astype(np.float16), mask=mask()),
        pa.array([decimal.Decimal(int(x)).scaleb(-2) for x in rng.integers(-10**15, 10**15, n)], type=pa.decimal128(30, 2), mask=mask()),
        pa.array(rng.random(n) < 0.5, mask=mask()),
        utf8_from_bytes([words[i] for i in rng.integers(0, len(words), n)], ~mask())],
        names=["p", "o", "i8", "i64", "f16", "dec", "b", "s"])
    items = []
    for col in ("i8", "i64", "f16", "dec", "b", "s"):
        for off in (0, 1, 7, T + 1, n + 5):
            items += [("lag", f"lag_{col}_{off}", col, "partition", off), ("lead", f"lead_{col}_{off}", col, "partition", off)]
    got = check(ctx, rec, ["p"], [("o", False, False)], items, device_in=True)
    nc = rec.num_columns
    assert got.column(nc).null_count == rec.column(2).null_count                      # offset 0: the row's own value
    assert 0 < got.column(nc + 6).null_count < n and got.column(nc + 8).null_count == n      # T + 1 reaches; past the partition never
    huge = [("lead", "far", "s", "partition", 2**63 - 1), ("lag", "far2", "b", "partition", 2**40)]
    got = check(ctx, rec, [], [], huge)
    assert got.column(nc).null_count == n and got.column(nc + 1).null_count == n


# ---- float sums --------------------------------------------------------------------------------------------------------------------
def test_float_sums_are_bit_identical_and_shared_by_peers(ctx):
    rng = np.random.default_rng(5)
    n = 50_000
    rec = pa.RecordBatch.from_arrays([pa.array(rng.integers(0, 7, n).astype(np.int32)), pa.array(rng.integers(0, 400, n).astype(np.int32)),
                                      pa.array(rng.standard_normal(n) * 10.0 ** rng.integers(-8, 8, n), mask=rng.random(n) < 0.1),
                                      pa.array(rng.standard_normal(n).astype(np.float32))], names=["p", "o", "v", "w"])
    items = [("sum", "rows", "v", "rows", 0), ("sum", "range", "v", "range", 0), ("sum", "all", "v", "partition", 0), ("sum", "w_range", "w", "range", 0)]
    p, o, it = W.to_plan(["p"], [("o", False, False)], items)
    dev = chq.DeviceRecordBatch.from_host(rec, ctx)
    runs = [chq.window_record(dev, aliases(rec), p, o, it, ctx=ctx).to_host() for _ in range(2)]
    runs.append(chq.window_record(rec, aliases(rec), p, o, it, ctx=ctx))
    compare(runs[0], *W.window(rec, ["p"], [("o", False, False)], items))
    for r in runs[1:]:
        for c in range(4, 8):
            assert bits(r.column(c).fill_null(0)) == bits(runs[0].column(c).fill_null(0)) and r.column(c).null_count == runs[0].column(c).null_count
    pk, ok = rec.column(0).to_numpy(), rec.column(1).to_numpy()
    for c, key in ((5, pk.astype(np.int64) * 1000 + ok), (7, pk.astype(np.int64) * 1000 + ok), (6, pk.astype(np.int64))):
        b = np.array(bits(runs[0].column(c).fill_null(0)), dtype=np.uint64)
        order = np.argsort(key, kind="stable")
        same = key[order][1:] == key[order][:-1]
        assert (b[order][1:][same] == b[order][:-1][same]).all(), c


def test_float_edge_values_and_exact_float32_sums(ctx):
    inf, nan = math.inf, math.nan
    parts = [[1.0, nan, 2.0], [inf, 1.0, -inf], [inf, 5.0, inf], [-inf, -1e300], [None, None, None], [None, 2.5, None], [-0.0, -0.0]]
    keys, vals = [], []
    for g, xs in enumerate(parts):
        keys += [g] * len(xs)
        vals += xs
    items = [("sum", "rows", "v", "rows", 0), ("sum", "all", "v", "partition", 0), ("count", "c", "v", "rows", 0), ("min", "lo", "v", "rows", 0),
             ("max", "hi", "v", "range", 0)]
    for t in (pa.float64(), pa.float32()):
        tv = [None if v is None else (v if t == pa.float64() or not abs(v) >= 1e38 or math.isinf(v) else math.copysign(1e38, v)) for v in vals]
        rec = pa.RecordBatch.from_arrays([pa.array(keys, type=pa.int32()), pa.array(np.arange(len(keys), dtype=np.int32)), pa.array(tv, type=t)],
                                         names=["k", "o", "v"])
        got = check(ctx, rec, ["k"], [("o", False, False)], items)
        s = got.column(3).to_pylist()
        assert s[0] == 1.0 and math.isnan(s[1]) and math.isnan(s[2]) and s[3:5] == [inf, inf] and math.isnan(s[5]) and s[6:9] == [inf, inf, inf]
        assert s[11:17] == [None, None, None, None, 2.5, 2.5] and math.copysign(1.0, s[17]) == -1.0 and s[18] == 0.0 and math.copysign(1.0, s[18]) == -1.0
    # a NaN in one tile reaches every later row of its partition, and no row of the next one
    n = 3 * T + 5
    big = np.ones(n)
    big[T - 3] = nan
    rec = pa.RecordBatch.from_arrays([pa.array((np.arange(n) >= 2 * T + 9).astype(np.int32)), pa.array(big)], names=["k", "v"])
    got = check(ctx, rec, ["k"], [], [("sum", "s", "v", "rows", 0)])
    s = got.column(2).to_numpy()
    assert np.isnan(s[T - 3:2 * T + 9]).all() and s[:T - 3].tolist() == list(range(1, T - 2)) and s[2 * T + 9:].tolist() == list(range(1, n - 2 * T - 8))
    # Float32 integers below 2^24: every partial sum is an integer below 2^53, so every order gives the exact total
    rng = np.random.default_rng(3)
    ints = rng.integers(0, 2**24, n)
    rec = pa.RecordBatch.from_arrays([pa.array(rng.integers(0, 3, n).astype(np.int32)), pa.array(ints.astype(np.float32))], names=["k", "v"])
    got = check(ctx, rec, ["k"], [], [("sum", "s", "v", "rows", 0)])
    k = rec.column(0).to_numpy()
    for g in range(3):
        assert got.column(2).to_numpy()[k == g].tolist() == np.cumsum(ints[k == g]).astype(np.float64).tolist()


# ---- integer overflow --------------------------------------------------------------------------------------------------------------
def test_integer_overflow_is_decided_on_the_exact_total_of_every_frame(ctx):
    i64max, u64max = 2**63 - 1, 2**64 - 1

    def batch(values, t):
        return pa.RecordBatch.from_arrays([pa.array(values, type=t), pa.array(np.arange(len(values), dtype=np.int32))], names=["v", "o"])

    order = [("o", False, False)]
    for values, t, total in (([i64max, 1, -5], pa.int64(), i64max - 4), ([-2**63, -1, 7], pa.int64(), -2**63 + 6)):
        rec = batch(values, t)
        assert check(ctx, rec, [], order, [("sum", "total", "v", "partition", 0)]).column(2).to_pylist() == [total] * 3
        with pytest.raises(SumOverflow):
            W.window(rec, [], order, [("sum", "total", "v", "rows", 0)])
        p, o, it = W.to_plan([], order, [("sum", "total", "v", "rows", 0)])
        for device_result in (False, True):
            with pytest.raises(chq.ChqError) as ei:
                chq.window_record(rec, aliases(rec), p, o, it, ctx=ctx, device_result=device_result)       # nothing comes back
            assert ei.value.code == 20 and "total" in str(ei.value), ei.value
    # UInt64 has no way back: the partition total is outside whenever a running total is; the running frame of the rows before is not
    rec = batch([u64max - 3, 1, 2, 1], pa.uint64())
    with pytest.raises(chq.ChqError) as ei:
        chq.window_record(rec, aliases(rec), *W.to_plan([], order, [("sum", "total", "v", "rows", 0)]), ctx=ctx)
    assert ei.value.code == 20 and "total" in str(ei.value) and "UInt64" in str(ei.value)
    assert check(ctx, batch([u64max - 3, 1, 2], pa.uint64()), [], order, [("sum", "total", "v", "rows", 0)]).column(2).to_pylist() == \
        [u64max - 3, u64max - 2, u64max]
    # the running total leaves the range in one tile and is back in another: ROWS fails, PARTITION does not
    n = 3 * T
    v = np.zeros(n, np.int64)
    v[[3, T + 1, 2 * T + 5]] = [i64max, i64max, -i64max]
    rec = pa.RecordBatch.from_arrays([pa.array(v), pa.array(np.arange(n, dtype=np.int32))], names=["v", "o"])
    assert check(ctx, rec, [], order, [("sum", "total", "v", "partition", 0)]).column(2).to_pylist() == [i64max] * n
    with pytest.raises(chq.ChqError) as ei:
        chq.window_record(rec, aliases(rec), *W.to_plan([], order, [("sum", "total", "v", "rows", 0)]), ctx=ctx)
    assert ei.value.code == 20
    # narrower inputs widen: they cannot overflow
    rec = batch(np.full(5000, 2**31 - 1, np.int32), pa.int32())
    assert check(ctx, rec, [], order, [("sum", "total", "v", "rows", 0)]).column(2).to_pylist()[-1] == 5000 * (2**31 - 1)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
PAYLOAD_ITEMS = [("row_number", "rn", None, "partition", 0), ("rank", "rk", None, "partition", 0), ("lag", "prev_s", "s", "partition", 1),
                 ("lead", "next_dec", "dec", "partition", 2), ("lag", "prev_fsb", "fsb4", "partition", 1), ("count", "cs", "s", "rows", 0),
                 ("count", "cb", "b", "range", 0), ("sum", "su8", "u8", "rows", 0), ("sum", "sf", "f64", "range", 0), ("min", "lo16", "f16", "rows", 0),
                 ("max", "ts", "ts", "partition", 0), ("count_star", "n", None, "rows", 0)]
PAYLOAD_ORDER = [("u8", True, False)]


@pytest.mark.parametrize("offset,length", [(1, 5000), (7, 3000), (64, 100), (4097, 2500), (13, 0)])
def test_sliced_device_views(ctx, offset, length):
    rng = np.random.default_rng(offset)
    parent = payload_batch(rng, 7000)
    dev = chq.DeviceRecordBatch.from_host(parent, ctx).slice(offset, length)
    view = parent.slice(offset, length)
    p, o, it = W.to_plan(["k"], PAYLOAD_ORDER, PAYLOAD_ITEMS)
    got = chq.window_record(dev, aliases(parent), p, o, it, ctx=ctx).to_host()
    compare(got, *W.window(view, ["k"], PAYLOAD_ORDER, PAYLOAD_ITEMS))
    for part, order in ((["b", "s"], [("f64", False, True)]), (["u8"], [("b", True, True), ("s", False, False)])):   # Boolean, Utf8 and null keys at the view's offset
        p, o, it = W.to_plan(part, order, PAYLOAD_ITEMS)
        got = chq.window_record(dev, aliases(parent), p, o, it, ctx=ctx).to_host()
        compare(got, *W.window(view, part, order, PAYLOAD_ITEMS))
    check(ctx, view, ["k"], PAYLOAD_ORDER, PAYLOAD_ITEMS, device_result=True)        # a sliced host view


def test_group_of_1000_batches_some_of_them_empty(ctx):
    rng = np.random.default_rng(4)
    batches = []
    for b in range(1000):
        n = 0 if b % 7 == 3 else int(rng.integers(1, 60))
        batches.append(pa.RecordBatch.from_arrays([pa.array(rng.integers(0, 50, n).astype(np.int32), mask=rng.random(n) < 0.05),
                                                   pa.array(["%02d" % v for v in rng.integers(0, 20, n)], type=pa.utf8()),
                                                   pa.array((rng.random(n) * 100).astype(np.float32), mask=rng.random(n) < 0.1),
                                                   pa.array(np.arange(n, dtype=np.int64) + 1000 * b)], names=["k", "s", "value2", "id"]))
    items = [("row_number", "rn", None, "partition", 0), ("dense_rank", "dr", None, "partition", 0), ("sum", "total", "value2", "range", 0),
             ("lag", "prev", "s", "partition", 1), ("max", "last", "id", "rows", 0)]
    order = [("s", False, False)]
    p, o, it = W.to_plan(["k"], order, items)
    exp = W.window_batches(batches, ["k"], order, items)
    got = chq.window_records(batches, aliases(batches[0]), p, o, it, ctx=ctx)
    compare(got, *exp)
    assert got.column(3).to_pylist() == [x for b in batches for x in b.column(3).to_pylist()]      # batch order, then row order
    dev = [chq.DeviceRecordBatch.from_host(b, ctx) for b in batches]
    got = chq.window_records(dev, aliases(batches[0]), p, o, it, ctx=ctx)
    assert isinstance(got, chq.DeviceRecordBatch)
    compare(got.to_host(), *exp)
    grp = chq.RecordGroup(dev, ctx)
    compare(chq.window_records(grp, aliases(batches[0]), p, o, it, ctx=ctx, device_result=False), *exp)
    other = pa.RecordBatch.from_arrays([pa.array([1, 2], type=pa.int64())], names=["k"])
    with pytest.raises(chq.ChqError) as ei:
        chq.window_records([batches[0], other], aliases(batches[0]), p, o, it, ctx=ctx)
    assert ei.value.code == 22


def test_host_and_device_inputs_and_outputs(ctx):
    rng = np.random.default_rng(10)
    rec = payload_batch(rng, 6000)
    exp = W.window(rec, ["k"], PAYLOAD_ORDER, PAYLOAD_ITEMS)
    p, o, it = W.to_plan(["k"], PAYLOAD_ORDER, PAYLOAD_ITEMS)
    dev = chq.DeviceRecordBatch.from_host(rec, ctx)
    for src in (rec, dev):
        for device_result in (None, False, True):
            got = chq.window_record(src, aliases(rec), p, o, it, ctx=ctx, device_result=device_result)
            on_device = (src is dev) if device_result is None else device_result
            assert isinstance(got, chq.DeviceRecordBatch) == on_device
            compare(got.to_host() if on_device else got, *exp)


def test_zero_rows_keep_the_full_schema(ctx):
    rec = payload_batch(np.random.default_rng(2), 10).slice(0, 0)
    for device_in in (False, True):
        got = check(ctx, rec, ["k"], PAYLOAD_ORDER, PAYLOAD_ITEMS, device_in=device_in)
        assert got.num_rows == 0 and got.schema.names == rec.schema.names + [it[1] for it in PAYLOAD_ITEMS]


# ---- errors --------------------------------------------------------------------------------------------------------------------------
def _format_of(col):
    """the Arrow C format string of a column (what the error message names)"""
    return {"f16": "e", "b": "b", "ts": "tsm:", "dec": "d:20,2", "s": "u", "fsb4": "w:4", "fsb16": "w:16"}[col]


def test_errors_leave_no_output(ctx):
    rec = payload_batch(np.random.default_rng(3), 100)
    al = aliases(rec)
    K, F = A.WindowKind, A.WindowFrame

    def fails(part, order, items, code, *mentions):
        with pytest.raises(chq.ChqError) as ei:
            chq.window_record(rec, al, part, order, items, ctx=ctx)
        assert ei.value.code == code, (part, order, items, ei.value)
        for m in mentions:
            assert m in str(ei.value), ei.value

    key, by = [A.ident("k")], [A.OrderByExpr(A.ident("u8"))]
    rn = [A.WindowItem(K.ROW_NUMBER, "rn")]
    unsupported = [(K.SUM, "f16"), (K.SUM, "b"), (K.SUM, "ts"), (K.SUM, "dec"), (K.SUM, "s"), (K.SUM, "fsb4"), (K.MIN, "s"), (K.MAX, "s"),
                   (K.MIN, "b"), (K.MAX, "dec"), (K.MIN, "fsb16")]
    for kind, col in unsupported:                                                              # exactly GROUP BY's cases
        for frame in F:
            fails(key, by, [A.WindowItem(kind, "x", A.ident(col), frame)], 30, f"'{col}'", f"'{_format_of(col)}'")
    fails(key, by, [A.WindowItem(K.SUM, "x", A.ident("nope"))], 7)                             # the evaluator's statuses
    fails(key, by, [A.WindowItem(K.LAG, "x", A.ident("nope"), F.PARTITION, 1)], 7)
    fails([A.ident("nope")], by, rn, 7)
    fails(key, [A.OrderByExpr(A.ident("nope"))], rn, 7)
    fails([A.compound("t", "k")], by, rn, 8)
    plus = A.binop(A.ident("k"), A.BinaryOperator.Plus, A.number("1"))
    fails([plus], by, rn, 30)                                                                  # an expression as a key
    fails(key, [A.OrderByExpr(plus)], rn, 30)
    fails([A.Nested(A.ident("k"))], by, rn, 30)
    fails(key, by, [A.WindowItem(K.SUM, "x", plus)], 30)                                       # ... and as an argument
    fails(key, by, [A.WindowItem(K.LEAD, "x", plus, F.PARTITION, 1)], 30)
    fails([A.ident("fsb16")], by, rn, 30, "'fsb16'", "'w:16'")                                 # key types without an order
    fails(key, [A.OrderByExpr(A.ident("fsb4"))], rn, 30, "'fsb4'", "'w:4'")
    fails(key, by, [], 22)                                                                     # an empty item list
    fails(key, by, [A.WindowItem(10, "x")], 22, "'x'")                                         # an unknown kind
    fails(key, by, [A.WindowItem(-1, "x")], 22)
    fails(key, by, [A.WindowItem(K.SUM, "x", A.ident("u8"), 3)], 22, "'x'")                    # an unknown frame
    fails(key, by, [A.WindowItem(K.COUNT_STAR, "x", None, -1)], 22)
    for kind in (K.LAG, K.LEAD, K.COUNT, K.SUM, K.MIN, K.MAX):                                 # a missing column
        fails(key, by, [A.WindowItem(kind, "x")], 22, "'x'")
    fails(key, by, [A.WindowItem(K.LAG, "x", A.ident("u8"), F.PARTITION, -1)], 22, "'x'")      # a negative offset
    fails(key, by, rn + [A.WindowItem(K.LEAD, "y", A.ident("u8"), F.PARTITION, -2**63)], 22, "'y'")
    # the frame of a ranking kind or of LAG / LEAD is ignored, whatever it holds
    got = chq.window_record(rec, al, key, by, [A.WindowItem(K.RANK, "r", None, 77), A.WindowItem(K.LAG, "l", A.ident("s"), -5, 1)], ctx=ctx)
    compare(got, *W.window(rec, ["k"], [("u8", False, False)], [("rank", "r", None, "partition", 0), ("lag", "l", "s", "partition", 1)]))
    # aliases resolve like compute_value's: t.k with an alias list naming t
    ta = [["t"] for _ in range(rec.num_columns)]
    got = chq.window_record(rec, ta, [A.compound("t", "k")], [A.OrderByExpr(A.compound("t", "u8"))],
                            [A.WindowItem(K.MAX, "m", A.compound("t", "u8"), F.ROWS_TO_CURRENT)], ctx=ctx)
    compare(got, *W.window(rec, ["k"], [("u8", False, False)], [("max", "m", "u8", "rows", 0)]))


# ---- the SQL statement, the plan, the operator and the device ----------------------------------------------------------------------
def test_window_operator_end_to_end_on_the_device():
    from chapterhouseqe_amd.operators import (ExchangeOperator, FilterOperatorTask, OperatorInstanceConfig, WindowOperatorTask,
                                              build_default_operator_task_registry)
    from chapterhouseqe_amd.sample_data import simple_batches
    from oracle import oracle as O
    batches = simple_batches(20_000, 2, 500)
    sel = parse_select("select id, row_number() over (partition by value1 order by value2 desc, id) as rn, "
                       "sum(value2) over (partition by value1 order by value2 desc, id rows between unbounded preceding and current row) running, "
                       "lag(id) over (partition by value1 order by value2 desc, id), value1, "
                       "count(*) over (partition by value1 order by value2 desc, id range between unbounded preceding and unbounded following) n "
                       "from t where id > 100")
    partition_by, order_by, items, projection = window_plan(sel)
    exs = [ExchangeOperator(f"operator_p{i}_exchange", [f"operator_p{i + 1}_producer"]) for i in range(3)]
    for rid, b in enumerate(batches):
        exs[0].send_record(rid, b, aliases(b))
    exs[0].producers_completed()
    reg = build_default_operator_task_registry("/tmp")
    ftask = FilterOperatorTask(sel.selection)
    assert reg.find_task_builder(ftask).build(OperatorInstanceConfig(1, "operator_p1_producer", 7, ftask), [exs[0]], exs[1])() is None
    exs[1].producers_completed()
    wtask = WindowOperatorTask(partition_by, order_by, items, projection, 1000)
    wrun = reg.find_task_builder(wtask).build(OperatorInstanceConfig(2, "operator_p2_producer", 7, wtask), [exs[1]], exs[2])
    assert wrun() is None
    exs[2].producers_completed()
    got = []
    while True:
        r = exs[2].get_next_record("operator_p3_producer", 1)
        if not isinstance(r, tuple):
            break
        got.append(r)
        exs[2].operator_completed_record_processing("operator_p3_producer", r[0])
    assert [r[0] for r in got] == list(range(len(got))) and wrun.task.records_sent == len(got) and exs[1].num_records() == 0
    filtered = R.join([O.filter_record(b, aliases(b), sel.selection) for b in batches])
    rp, ro, ri = W.from_plan(partition_by, order_by, items)
    full, bounds = W.window(filtered, rp, ro, ri)
    names = ["id", "rn", "running", "lag(id)", "value1", "n"]
    exp = O.project_record(projection, full, aliases(full))           # the statement's SELECT list over the reference's columns
    assert exp.schema.names == names
    assert len(got) == -(-exp.num_rows // 1000) and wrun.task.rows_out == exp.num_rows == wrun.task.rows_in
    parts = [r[1].to_host() if isinstance(r[1], chq.DeviceRecordBatch) else r[1] for r in got]
    compare(R.join(parts), exp, {names.index(full.schema.names[c]): v for c, v in bounds.items()})
