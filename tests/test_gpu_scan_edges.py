"""GPU: the shared scan pieces of chapterhouseqe_amd/csrc/scan_device.h and scan.hip at the row counts where a tile or a round
of tile totals ends: 1 row, one row short of a tile, a full tile, a tile and a row, and one row past a full round of 256 tiles.
Each row count goes through the four users of the shared code -- the offsets scan under `||` and under the joins, the Utf8
gather of ORDER BY, the count rows of hash partitioning -- and the complete result is compared, bit for bit, with the host
reference the sibling GPU tests use.  Rows are drawn from small pools, so the references stay cheap."""
import numpy as np
import pyarrow as pa
import pytest

import chapterhouseqe_amd as chq
from chapterhouseqe_amd.sqlparse import parse_expr

from . import join_reference as J
from . import outer_join_reference as OJ
from . import partition_reference as P
from . import sort_reference as R
from .test_gpu_join import aliases, int_side, same, to_host
from .test_gpu_rounds import byte_total, offsets_of, payload_strings, same_array, utf8_pool
from .test_gpu_sort import explain, identical, ob

pytestmark = pytest.mark.gpu

T = 2048                                     # kScanTile
SIZES = [1, T - 1, T, T + 1, 256 * T + 1]    # 256 * T: one round of scan_totals_in_place
KK = [("k", "k")]


@pytest.fixture(scope="module")
def ctx():
    c = chq.Context(0)
    yield c
    c.close()


# ---- the offsets scan under the string functions: offsets, the trailing total, the bytes --------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_concat_of_short_strings_on_a_sliced_view(ctx, n):
    rng = np.random.default_rng(n)
    lead = 5
    pool = [b"", b"a", b"bc", b"def", b"\xc3\xa9", b"g", None]
    idx = rng.integers(0, len(pool), n + lead)
    idx[0], idx[lead], idx[-1] = 3, 3, 2                                     # (bytes before the view, a valid row at either end)
    if n > 2:
        idx[lead + n // 2] = len(pool) - 1
    s = utf8_pool(pool).take(pa.array(idx))
    dev = chq.DeviceRecordBatch.from_host(pa.RecordBatch.from_arrays([s], names=["s"]), ctx).slice(lead, n)
    assert offsets_of(s.slice(lead))[0] != 0
    got, is_scalar = chq.compute_value(dev, [[]], parse_expr("s || 'x'"), ctx=ctx)
    assert not is_scalar
    exp = utf8_pool([None if c is None else c + b"x" for c in pool]).take(pa.array(idx[lead:]))
    same_array(got, exp, f"s || 'x' over {n} rows")
    assert int(offsets_of(got)[-1]) == byte_total(exp) >= n // 2


# ---- the offsets scan under the joins -----------------------------------------------------------------------------------------
def small_side(row_name):
    """keys 2 and 3 once, 4 and 5 twice, one key nobody else holds and a null; keys 0 and 1 are absent"""
    return int_side([2, 4, 99, 3, 5, 4, 5, 0], row_name, np.array([False] * 7 + [True]))


def large_side(rng, n, row_name):
    """n rows over the keys 0 .. 5, a tenth of them null: 0, 1 or 2 rows of small_side match each"""
    return int_side(rng.integers(0, 6, n), row_name, rng.random(n) < 0.1)


def joined(ctx, left, right, how):
    got = to_host(chq.join_records(chq.DeviceRecordBatch.from_host(left, ctx), aliases(left), chq.DeviceRecordBatch.from_host(right, ctx),
                                   aliases(right), J.to_plan(KK), ctx=ctx, how=how))
    same(got, (J.join(left, right, KK) if how == "inner" else OJ.join(left, right, KK, how))[2])
    return got


@pytest.mark.parametrize("how", ["inner", "full"])
@pytest.mark.parametrize("n", SIZES)
def test_join_of_n_left_rows(ctx, n, how):
    rng = np.random.default_rng(2 * n)
    got = joined(ctx, large_side(rng, n, "lrow"), small_side("rrow"), how)
    assert got.num_rows >= (n if how == "full" else n // 2)


@pytest.mark.parametrize("n", SIZES)
def test_full_join_of_n_right_rows(ctx, n):
    """FULL's tail: the scan runs over the flags of the n right rows"""
    rng = np.random.default_rng(2 * n + 1)
    got = joined(ctx, small_side("lrow"), large_side(rng, n, "rrow"), "full")
    tail = ~np.asarray(got.column("lrow").is_valid())
    assert got.num_rows >= n and (n < T or int(tail.sum()) >= n // 4)


# ---- ORDER BY: the Utf8 gather ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_order_by_int32_with_a_utf8_payload(ctx, n):
    rng = np.random.default_rng(3 * n)
    pool = payload_strings(rng, 100)
    rec = pa.RecordBatch.from_arrays([pa.array(rng.integers(-3, 4, n).astype(np.int32), mask=rng.random(n) < 0.1),
                                      utf8_pool(pool).take(pa.array(rng.integers(0, len(pool), n))),
                                      pa.array(np.arange(n, dtype=np.int32))], names=["k", "s", "row"])
    keys = [("k", False, False)]
    got = chq.sort_record(chq.DeviceRecordBatch.from_host(rec, ctx), aliases(rec), ob(keys), ctx=ctx).to_host()
    exp = R.sort_batch(rec, keys)
    assert identical(got, exp), explain(got, exp)
    assert int(offsets_of(got.column("s"))[-1]) == byte_total(exp.column("s"))


# ---- hash partitioning: the count rows ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_partition_into_three(ctx, n):
    rng = np.random.default_rng(4 * n)
    values = pa.array(np.arange(-50, 50, dtype=np.int32) * 40_000_003, mask=np.arange(100) == 17)
    idx = rng.integers(0, len(values), n)
    rec = pa.RecordBatch.from_arrays([values.take(pa.array(idx)), pa.array(np.arange(n, dtype=np.int32))], names=["k", "row"])
    ids = P.ids_of_hashes(P.row_hashes(pa.RecordBatch.from_arrays([values], names=["k"]), ["k"])[idx], 3)
    order = np.argsort(ids, kind="stable")                                   # rows in input order inside every partition
    cuts = np.searchsorted(ids[order], np.arange(4))
    got = chq.partition_records(chq.DeviceRecordBatch.from_host(rec, ctx), aliases(rec), P.to_plan(["k"]), 3, ctx=ctx)
    assert len(got) == 3
    for p in range(3):
        same(got[p].to_host(), rec.take(pa.array(order[cuts[p]:cuts[p + 1]])))
    assert n < T or all(g.num_rows > 0 for g in got)
