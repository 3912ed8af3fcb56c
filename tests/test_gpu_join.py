"""GPU: INNER JOIN (chq_join_records) compared exactly -- row order, NaN payloads and null counts included -- with the host
reference of tests/join_reference.py (itself pinned to the filtered cross product by tests/test_join_host.py)."""
import numpy as np
import pyarrow as pa
import pytest

import chapterhouseqe_amd as chq
from chapterhouseqe_amd import sqlast as A
from chapterhouseqe_amd.sqlparse import join_plan, parse_select

from . import join_reference as J
from . import sort_reference as R
from .helpers import arrays_identical
from .test_gpu_sort import KINDS, explain, float_bits, identical, key_array, payload_batch, utf8_from_bytes

pytestmark = pytest.mark.gpu

T = 2048   # sorted positions, left rows and output rows per workgroup tile (join_device.h kJoinTile)
SIZES = [0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 5]


@pytest.fixture(scope="module")
def ctx():
    return chq.Context(0)


def aliases(rec):
    return [[] for _ in range(rec.num_columns)]


def to_host(got):
    return got.to_host() if isinstance(got, chq.DeviceRecordBatch) else got


def same(got, exp):
    """every column with arrays_identical (FixedSizeBinary columns by value), fields included"""
    assert identical(got, exp), explain(got, exp)
    for i in range(exp.num_columns):
        if not pa.types.is_fixed_size_binary(exp.column(i).type):
            assert arrays_identical(got.column(i), exp.column(i)), exp.schema.field(i).name


def check(ctx, left, right, keys, device_in=False, device_result=None):
    """one join of two host batches against the reference; returns the result (on the host)"""
    ls = chq.DeviceRecordBatch.from_host(left, ctx) if device_in else left
    rs = chq.DeviceRecordBatch.from_host(right, ctx) if device_in else right
    got = chq.join_records(ls, aliases(left), rs, aliases(right), J.to_plan(keys), ctx=ctx, device_result=device_result)
    assert isinstance(got, chq.DeviceRecordBatch) == (device_in if device_result is None else device_result)
    got = to_host(got)
    same(got, J.join(left, right, keys)[2])
    return got


def int_side(keys, row_name, mask=None):
    keys = np.asarray(keys, dtype=np.int32)
    return pa.RecordBatch.from_arrays([pa.array(keys, mask=mask), pa.array(np.arange(len(keys), dtype=np.int32))], names=["k", row_name])


def pooled_side(rng, n, pool, row_name):
    """n rows whose keys come from about `pool` values, 15 % of them null"""
    return int_side(rng.integers(0, max(1, pool), n), row_name, rng.random(n) < 0.15)


# ---- row counts ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nl", SIZES)
def test_row_counts(ctx, nl):
    rng = np.random.default_rng(nl)
    for nr in SIZES:
        pool = max(nl, nr) // 4
        left, right = pooled_side(rng, nl, pool, "lrow"), pooled_side(rng, nr, pool, "rrow")
        got = check(ctx, left, right, [("k", "k")], device_in=(nl + nr) % 2 == 1)
        s = ctx.last_stats()
        assert s["rows_in"] == nl + nr and s["rows_out"] == got.num_rows
        if nl >= 64 and nr >= 64:
            assert 0 < got.num_rows < nl * nr, (nl, nr)          # (no case passes vacuously)
        if nl == 0 or nr == 0:
            assert got.num_rows == 0 and got.schema == pa.schema(list(left.schema) + list(right.schema))


# ---- shapes ---------------------------------------------------------------------------------------------------------------------
def test_all_keys_distinct_one_to_one(ctx):
    rng = np.random.default_rng(1)
    n = 3 * T + 5
    got = check(ctx, int_side(rng.permutation(n), "lrow"), int_side(rng.permutation(n), "rrow"), [("k", "k")])
    assert got.num_rows == n and got.column(1).to_pylist() == list(range(n))


@pytest.mark.parametrize("nl,nr", [(65, 65), (T + 1, 3), (3, T + 1)])
def test_one_key_everywhere(ctx, nl, nr):
    got = check(ctx, int_side(np.full(nl, 7), "lrow"), int_side(np.full(nr, 7), "rrow"), [("k", "k")], device_in=True)
    assert got.num_rows == nl * nr
    assert got.column(1).to_pylist() == np.repeat(np.arange(nl), nr).tolist()          # left-major
    assert got.column(3).to_pylist() == np.tile(np.arange(nr), nl).tolist()


def test_one_left_row_matching_many_right_rows(ctx):
    n = 3 * T + 5
    left = int_side([1, 5, 2], "lrow")
    got = check(ctx, left, int_side(np.full(n, 5), "rrow"), [("k", "k")])
    assert got.num_rows == n and set(got.column(1).to_pylist()) == {1} and got.column(3).to_pylist() == list(range(n))


def test_unmatched_left_rows_between_two_matching_ones(ctx):
    left = int_side([1] + list(range(100, 100 + T + 1)) + [1], "lrow")
    right = int_side([1, 9, 1, 1], "rrow")
    got = check(ctx, left, right, [("k", "k")])
    assert got.column(1).to_pylist() == [0, 0, 0, T + 2, T + 2, T + 2] and got.column(3).to_pylist() == [0, 2, 3] * 2


@pytest.mark.parametrize("right_run", [T - 1, T, T + 1, 2 * T])
def test_split_on_a_tile_boundary_of_the_sorted_positions(ctx, right_run):
    """key 0 is the first run of the sorted positions: its right rows fill positions [0, right_run), its left rows follow"""
    left = int_side([3, 0, 1, 0, 2, 0, 1], "lrow")
    right = int_side([0] * right_run + [1, 1, 1, 4], "rrow")
    got = check(ctx, left, right, [("k", "k")], device_in=True)
    assert got.num_rows == 3 * right_run + 2 * 3
    # ... and a run that has no left rows, ending on the boundary, in front of one that has no right rows
    check(ctx, int_side([1, 1, 2], "lrow"), int_side([0] * right_run + [2], "rrow"), [("k", "k")])


def test_matches_only_in_the_first_and_the_last_left_row(ctx):
    n = 3 * T + 5
    keys = np.arange(1000, 1000 + n)
    keys[0] = keys[-1] = 5
    got = check(ctx, int_side(keys, "lrow"), int_side([5, 6, 5], "rrow"), [("k", "k")])
    assert got.column(1).to_pylist() == [0, 0, n - 1, n - 1]


def test_all_keys_null_on_one_side(ctx):
    rng = np.random.default_rng(2)
    n = T + 7
    full = pooled_side(rng, n, 50, "row")
    nulls = pa.RecordBatch.from_arrays([pa.array([None] * n, type=pa.int32()), full.column(1)], names=["k", "row"])
    assert check(ctx, nulls, full, [("k", "k")]).num_rows == 0
    assert check(ctx, full, nulls, [("k", "k")], device_in=True).num_rows == 0
    assert check(ctx, nulls, nulls, [("k", "k")]).num_rows == 0          # a null matches nothing, a null included


# ---- key types --------------------------------------------------------------------------------------------------------------------
def keyed(keys, row_name):
    return pa.RecordBatch.from_arrays([keys, pa.array(np.arange(len(keys), dtype=np.int32))], names=["k", row_name])


@pytest.mark.parametrize("kind", KINDS)
def test_every_key_type(ctx, kind):
    rng = np.random.default_rng(100 + KINDS.index(kind))
    pool = key_array(rng, 300, kind, True)          # both sides draw from one pool of values (nulls among them): matches exist
    left = keyed(pool.take(pa.array(rng.integers(0, 300, 2500))), "lrow")
    right = keyed(pool.take(pa.array(rng.integers(0, 300, 1500))), "rrow")
    got = check(ctx, left, right, [("k", "k")], device_in=kind in ("float32", "utf8", "decimal"))
    assert 0 < got.num_rows < 2500 * 1500
    assert got.column(0).null_count == 0 and got.column(2).null_count == 0


@pytest.mark.parametrize("width", [2, 4, 8])
def test_float_keys_match_by_bits(ctx, width):
    rng = np.random.default_rng(width)
    left, right = keyed(float_bits(rng, 3000, width), "lrow"), keyed(float_bits(rng, 2000, width), "rrow")
    got = check(ctx, left, right, [("k", "k")])
    ut = {2: np.uint16, 4: np.uint32, 8: np.uint64}[width]
    lb = got.column(0).to_numpy(zero_copy_only=False).view(ut)
    rb = got.column(2).to_numpy(zero_copy_only=False).view(ut)
    assert got.num_rows > 0 and np.array_equal(lb, rb)
    sign = 1 << (8 * width - 1)
    assert {int(x) for x in lb if int(x) & (sign - 1) == 0} == {0, sign}          # +0 and -0 both matched, each only itself


def test_utf8_keys_prefixes_empty_strings_nuls_and_long_strings(ctx):
    rng = np.random.default_rng(9)
    base = []
    for plen in (0, 7, 8, 9, 33, 64, 300):
        p = bytes(rng.integers(97, 100, plen).astype(np.uint8))
        base += [p, p + b"\x00", p + b"a", p + b"b", p + b"\x00\x00", p + b"a\x00", p + b"ab"]
    base += [b"", b"\x00", b"\xe2\x82\xac"]

    def side(n, row_name):
        vals = [base[i] for i in rng.integers(0, len(base), n)]
        return keyed(utf8_from_bytes(vals, rng.random(n) < 0.85), row_name)          # "" and null both occur

    got = check(ctx, side(3000, "lrow"), side(2000, "rrow"), [("k", "k")])
    assert got.num_rows > 0 and "" in got.column(0).to_pylist()
    check(ctx, side(500, "lrow"), side(T + 1, "rrow"), [("k", "k")], device_in=True)


# ---- key counts -------------------------------------------------------------------------------------------------------------------
def test_two_keys_of_mixed_types(ctx):
    rng = np.random.default_rng(21)

    def side(n, row_name):
        return pa.RecordBatch.from_arrays([
            pa.array([["x", "y", "xy", ""][i] for i in rng.integers(0, 4, n)], mask=rng.random(n) < 0.1),
            pa.array(rng.choice([0.0, -0.0, np.nan, 1.0], n).astype(np.float64), mask=rng.random(n) < 0.1),
            pa.array(np.arange(n, dtype=np.int32))], names=["s", "f", row_name])

    left, right = side(3000, "lrow"), side(2500, "rrow")
    got = check(ctx, left, right, [("s", "s"), ("f", "f")])
    assert 0 < got.num_rows < J.join(left, right, [("s", "s")])[2].num_rows
    check(ctx, left, right, [("f", "f"), ("s", "s")], device_in=True)


def test_nine_keys_take_two_head_launches(ctx):
    rng = np.random.default_rng(22)

    def side(n, row_name):
        cols = [pa.array(rng.integers(0, 2, n).astype(np.int8), mask=(rng.random(n) < 0.05) if i in (0, 8) else None) for i in range(9)]
        return pa.RecordBatch.from_arrays(cols + [pa.array(np.arange(n, dtype=np.int32))], names=[f"k{i}" for i in range(9)] + [row_name])

    left, right = side(3000, "lrow"), side(2000, "rrow")
    keys = [(f"k{i}", f"k{i}") for i in range(9)]
    got = check(ctx, left, right, keys)
    assert 0 < got.num_rows < J.join(left, right, keys[:8])[2].num_rows          # the ninth key and its nulls count


def test_keys_of_more_rows_than_one_concat_slice(ctx):
    """the key columns of a side are concatenated in slices of 16 384 rows or more: Utf8, Boolean and nullable keys across
    several of them, on sides whose own views are sliced at odd offsets"""
    rng = np.random.default_rng(23)

    def side(n, row_name):
        return pa.RecordBatch.from_arrays([
            pa.array(["s%d" % i * (1 + i % 3) for i in rng.integers(0, 20_000, n)], mask=rng.random(n) < 0.1),
            pa.array(rng.random(n) < 0.5, mask=rng.random(n) < 0.1),
            pa.array(rng.choice([0.0, -0.0, 1.0], n).astype(np.float64)),
            pa.array(np.arange(n, dtype=np.int32))], names=["s", "b", "f", row_name])

    lp, rp = side(40_003, "lrow"), side(35_011, "rrow")
    keys = [("s", "s"), ("b", "b"), ("f", "f")]
    got = check(ctx, lp, rp, keys)
    assert 0 < got.num_rows < 40_003 * 35_011
    lv = chq.DeviceRecordBatch.from_host(lp, ctx).slice(3, 40_000)
    rv = chq.DeviceRecordBatch.from_host(rp, ctx).slice(9, 35_000)
    got = chq.join_records(lv, aliases(lp), rv, aliases(rp), J.to_plan(keys), ctx=ctx).to_host()
    same(got, J.join(lp.slice(3, 40_000), rp.slice(9, 35_000), keys)[2])


# ---- payloads and inputs ----------------------------------------------------------------------------------------------------------
def test_payload_of_every_importable_type_on_both_sides(ctx):
    rng = np.random.default_rng(33)
    left, right = payload_batch(rng, 700), payload_batch(rng, 600)
    got = check(ctx, left, right, [("k", "k")])
    assert got.num_rows > 700 and got.schema.names == left.schema.names + right.schema.names
    check(ctx, left, right, [("k", "k"), ("b2", "b2")], device_in=True, device_result=False)
    check(ctx, left, right, [("u8", "u8")], device_in=False, device_result=True)


@pytest.mark.parametrize("offset,length", [(1, 3000), (9, 2049), (64, 100), (13, 0)])
def test_sliced_device_views(ctx, offset, length):
    rng = np.random.default_rng(offset)
    lp, rp = payload_batch(rng, 4000), payload_batch(rng, 900)
    lv = chq.DeviceRecordBatch.from_host(lp, ctx).slice(offset, length)
    rv = chq.DeviceRecordBatch.from_host(rp, ctx).slice(7, 800)
    for keys in ([("k", "k")], [("s", "s"), ("b", "b")]):
        got = chq.join_records(lv, aliases(lp), rv, aliases(rp), J.to_plan(keys), ctx=ctx).to_host()
        same(got, J.join(lp.slice(offset, length), rp.slice(7, 800), keys)[2])
    got = chq.join_records(lp.slice(offset, length), aliases(lp), rp.slice(7, 800), aliases(rp), J.to_plan([("u8", "u8")]), ctx=ctx)
    same(got, J.join(lp.slice(offset, length), rp.slice(7, 800), [("u8", "u8")])[2])


def test_groups_of_50_batches_with_empty_batches_and_mixed_residency(ctx):
    rng = np.random.default_rng(8)
    lp, rp = payload_batch(rng, 5000), payload_batch(rng, 3000)

    def windows(n):
        cuts = np.sort(rng.integers(0, n, 49)).tolist()
        cuts[10] = cuts[9]
        cuts[30] = cuts[29]          # empty batches
        return list(zip([0] + cuts, cuts + [n]))

    lw, rw = windows(5000), windows(3000)
    lh, rh = [lp.slice(a, b - a) for a, b in lw], [rp.slice(a, b - a) for a, b in rw]
    ld, rd = chq.DeviceRecordBatch.from_host(lp, ctx), chq.DeviceRecordBatch.from_host(rp, ctx)
    lmix = [ld.slice(a, b - a) if i % 3 else lh[i] for i, (a, b) in enumerate(lw)]
    rmix = [rh[i] if i % 2 else rd.slice(a, b - a) for i, (a, b) in enumerate(rw)]
    assert len(lmix) == 50 and any(b.num_rows == 0 for b in lh)
    keys = [("k", "k"), ("b2", "b2")]
    exp = J.join(lh, rh, keys)[2]
    got = chq.join_records(lmix, aliases(lp), rmix, aliases(rp), J.to_plan(keys), ctx=ctx)
    assert isinstance(got, pa.RecordBatch)          # not every input on the device: a host result
    same(got, exp)
    got = chq.join_records(lh, aliases(lp), [rd.slice(a, b - a) for a, b in rw], aliases(rp), J.to_plan(keys), ctx=ctx, device_result=True)
    same(got.to_host(), exp)


def test_record_group_inputs_and_device_result_both_ways(ctx):
    rng = np.random.default_rng(12)
    lp, rp = payload_batch(rng, 3000), payload_batch(rng, 1000)
    lh, rh = [lp.slice(0, 1000), lp.slice(1000, 2000)], [rp.slice(0, 1), rp.slice(1, 999)]
    keys = [("k", "k")]
    exp = J.join(lh, rh, keys)[2]
    ld = chq.DeviceRecordBatch.from_host(lp, ctx)
    lgrp, rgrp = chq.RecordGroup([ld.slice(0, 1000), ld.slice(1000, 2000)], ctx), chq.RecordGroup(rh, ctx)
    got = chq.join_records(lgrp, aliases(lp), rgrp, aliases(rp), J.to_plan(keys), ctx=ctx)
    same(got, exp)
    got = chq.join_records(lgrp, aliases(lp), rgrp, aliases(rp), J.to_plan(keys), ctx=ctx, device_result=True)          # groups are reusable
    assert isinstance(got, chq.DeviceRecordBatch)
    same(got.to_host(), exp)
    rgrp.release()
    got = chq.join_records(lgrp, aliases(lp), chq.DeviceRecordBatch.from_host(rp, ctx), aliases(rp), J.to_plan(keys), ctx=ctx)
    assert isinstance(got, chq.DeviceRecordBatch)          # every input on the device: a device result
    same(got.to_host(), exp)
    same(chq.join_records(lgrp, aliases(lp), rp, aliases(rp), J.to_plan(keys), ctx=ctx, device_result=False), exp)


# ---- against the product's own filter ---------------------------------------------------------------------------------------------
def test_join_is_the_filtered_cross_product(ctx):
    rng = np.random.default_rng(40)
    left = pa.RecordBatch.from_arrays([pa.array(rng.integers(0, 8, 40).astype(np.int32), mask=rng.random(40) < 0.2),
                                       pa.array(np.arange(40, dtype=np.int32)), pa.array([f"l{i}" for i in range(40)], mask=rng.random(40) < 0.3)],
                                      names=["k", "lrow", "tag"])
    right = pa.RecordBatch.from_arrays([pa.array(rng.integers(0, 8, 50).astype(np.int32), mask=rng.random(50) < 0.2),
                                        pa.array(np.arange(50, dtype=np.int32)), pa.array((rng.random(50) * 10).astype(np.float32))],
                                       names=["k", "rrow", "x"])
    la, ra = [["l"]] * 3, [["r"]] * 3
    on = A.binop(A.compound("l", "k"), A.BinaryOperator.Eq, A.compound("r", "k"))
    exp = chq.filter_record(J.cross_product(left, right), la + ra, on, ctx=ctx)
    got = chq.join_records(left, la, right, ra, [(A.compound("l", "k"), A.compound("r", "k"))], ctx=ctx)
    assert 0 < exp.num_rows < 2000
    same(got, exp)


def test_two_calls_give_bit_identical_results(ctx):
    rng = np.random.default_rng(41)
    left, right = payload_batch(rng, 5000), payload_batch(rng, 4000)
    keys = J.to_plan([("k", "k"), ("b2", "b2")])
    a = chq.join_records(left, aliases(left), right, aliases(right), keys, ctx=ctx)
    b = chq.join_records(left, aliases(left), right, aliases(right), keys, ctx=ctx)
    assert a.num_rows > 5000
    same(a, b)


def test_stats(ctx):
    rng = np.random.default_rng(42)
    left, right = pooled_side(rng, 5000, 100, "lrow"), pooled_side(rng, 3000, 100, "rrow")
    got = check(ctx, left, right, [("k", "k")])
    s = ctx.last_stats()
    assert s["rows_in"] == 8000 and s["rows_out"] == got.num_rows > 0 and s["launches"] > 0
    assert s["bytes_read_alg"] > 0 and s["bytes_written_alg"] >= got.num_rows * 16


# ---- errors ---------------------------------------------------------------------------------------------------------------------------
def test_errors_leave_no_output(ctx):
    rng = np.random.default_rng(3)
    left, right = payload_batch(rng, 100), payload_batch(rng, 80)
    la, ra = aliases(left), aliases(right)
    k = A.ident("k")
    plus = A.binop(A.ident("k"), A.BinaryOperator.Plus, A.number("1"))
    cases = [([], 22, ""),                                                   # no keys: there is no cross join
             ([(k, A.ident("u8"))], 30, ""),                                 # Int16 with UInt8: no coercion
             ([(A.ident("nope"), k)], 7, ""),
             ([(k, A.ident("nope"))], 7, ""),
             ([(A.compound("t", "k"), k)], 8, ""),
             ([(plus, k)], 30, ""), ([(k, plus)], 30, ""), ([(A.Nested(k), k)], 30, ""),
             ([(A.ident("fsb16"), A.ident("fsb16"))], 30, "fsb16"),
             ([(k, k), (A.ident("fsb4"), A.ident("fsb4"))], 30, "fsb4")]
    for keys, code, word in cases:
        with pytest.raises(chq.ChqError) as ei:
            chq.join_records(left, la, right, ra, keys, ctx=ctx)
        assert ei.value.code == code and word in str(ei.value), (keys, ei.value)
    with pytest.raises(chq.ChqError) as ei:
        chq.join_records(left, la, right, ra, [(k, A.ident("u8"))], ctx=ctx)
    msg = str(ei.value)
    assert "'k'" in msg and "'u8'" in msg and "'s'" in msg and "'C'" in msg          # both columns, both types
    other = pa.RecordBatch.from_arrays([pa.array([1, 2], type=pa.int64())], names=["k"])
    with pytest.raises(chq.ChqError) as ei:
        chq.join_records([left, other], la, right, ra, [(k, k)], ctx=ctx)
    assert ei.value.code == 22
    # aliases resolve like compute_value's, each side against its own
    got = chq.join_records(left, [["l"]] * left.num_columns, right, [["r"]] * right.num_columns,
                           [(A.compound("l", "k"), A.compound("r", "k"))], ctx=ctx)
    same(got, J.join(left, right, [("k", "k")])[2])


def test_an_output_of_2_to_the_32_rows_is_refused(ctx):
    """65 536 x 65 536 equal keys: the total is exactly 2^32 and only fits a 64-bit count"""
    n = 1 << 16
    side = pa.RecordBatch.from_arrays([pa.array(np.full(n, 7, np.int8))], names=["k"])
    with pytest.raises(chq.ChqError) as ei:
        chq.join_records(side, [[]], side, [[]], J.to_plan([("k", "k")]), ctx=ctx)
    assert ei.value.code == 30 and str(1 << 32) in str(ei.value)
    # one row fewer on one side fits
    got = chq.join_records(side.slice(0, 1), [[]], side, [[]], J.to_plan([("k", "k")]), ctx=ctx)
    assert got.num_rows == n


# ---- scale, SQL, the operator -----------------------------------------------------------------------------------------------------
def test_200_000_by_200_000_rows(ctx):
    rng = np.random.default_rng(77)
    n = 200_000
    left = pa.RecordBatch.from_arrays([pa.array(rng.integers(0, 100_000, n).astype(np.int32)), pa.array(np.arange(n, dtype=np.int32)),
                                       pa.array((rng.random(n) * 100).astype(np.float32))], names=["k", "lrow", "v"])
    right = pa.RecordBatch.from_arrays([pa.array(rng.integers(0, 100_000, n).astype(np.int32), mask=rng.random(n) < 0.05),
                                        pa.array(np.arange(n, dtype=np.int32))], names=["k", "rrow"])
    got = check(ctx, left, right, [("k", "k")], device_in=True)
    assert 300_000 < got.num_rows < 500_000


def test_parsed_sql(ctx):
    from chapterhouseqe_amd.sample_data import simple_batches
    sel = parse_select("select * from read_files('facts/*.parquet') f inner join read_files('dims/*.parquet') as d "
                       "on d.id = f.id and f.value1 = d.value1 where f.id > 10")
    keys = join_plan(sel)
    facts = simple_batches(3000, 2, 700)
    dims = [b.slice(5, 300) for b in simple_batches(3000, 2, 1000)]
    fa, da = [["f"]] * 3, [["d"]] * 3
    got = chq.join_records(facts, fa, dims, da, keys, ctx=ctx)
    exp = J.join(facts, dims, J.from_plan(keys))[2]
    assert exp.num_rows == 900
    same(got, exp)
    kept = chq.filter_record(got, fa + da, sel.selection, ctx=ctx)          # the WHERE clause resolves f.id through the output aliases
    assert kept.num_rows == sum(1 for i in exp.column(0).to_pylist() if i > 10) > 800


def test_join_operator_end_to_end_on_the_device():
    from chapterhouseqe_amd.operators import ExchangeOperator, JoinOperatorTask, OperatorInstanceConfig, build_default_operator_task_registry
    from chapterhouseqe_amd.sample_data import simple_batches
    keys = join_plan(parse_select("select * from read_files('a') l join read_files('b') r on l.id = r.id"))
    left = simple_batches(20_000, 2, 500)
    rng = np.random.default_rng(6)
    right = [pa.RecordBatch.from_arrays([pa.array(rng.integers(0, 30_000, 4000).astype(np.int32)), pa.array(np.arange(o, o + 4000, dtype=np.int64))],
                                        names=["id", "n"]) for o in (0, 4000)]
    ex_l = ExchangeOperator("operator_l_exchange", ["operator_join_producer"])
    ex_r = ExchangeOperator("operator_r_exchange", ["operator_join_producer"])
    ex_out = ExchangeOperator("operator_join_exchange", ["operator_p2_producer"])
    for ex, batches, alias in ((ex_l, left, "l"), (ex_r, right, "r")):
        for rid, b in enumerate(batches):
            ex.send_record(rid, b, [[alias]] * b.num_columns)
        ex.producers_completed()
    task = JoinOperatorTask(keys, 1000)
    run = build_default_operator_task_registry("/tmp").find_task_builder(task).build(
        OperatorInstanceConfig(1, "operator_join_producer", 7, task), [ex_l, ex_r], ex_out)
    assert run() is None
    ex_out.producers_completed()
    got = []
    while True:
        r = ex_out.get_next_record("operator_p2_producer", 1)
        if not isinstance(r, tuple):
            break
        got.append(r)
        ex_out.operator_completed_record_processing("operator_p2_producer", r[0])
    exp = J.join(left, right, [("id", "id")])[2]
    assert exp.num_rows > 4000 and len(got) == -(-exp.num_rows // 1000) and [r[0] for r in got] == list(range(len(got)))
    assert all(r[2] == [["l"]] * 3 + [["r"]] * 2 for r in got)
    assert ex_l.num_records() == 0 and ex_r.num_records() == 0 and run.task.rows_out == exp.num_rows
    same(R.join([to_host(r[1]) for r in got]), exp)
