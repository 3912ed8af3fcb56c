"""GPU: the Parquet page encoder (csrc/parquet_write.hip, parquet_write.cpp) on batches built against its own units -- the
16-byte chunk and 128-byte stride of the string scatter, the 64-lane prefix, the 256-row step, the 4096-row block of the
scan, the page boundary, the bit offset of a view -- and on the values its statistics reduce from sentinels.

Every image is written twice (byte-equal: the statistics come from atomics and a candidate reduction) from a host batch and
from a device batch, and read three ways: by pyarrow, by this library's scan, and page by page by tests/parquet_unpage.py,
which also asserts what a reader may rely on (sizes, tiling, value counts).  All three are compared bit for bit with the input
(NaN payloads count), and page k of a chunk must hold rows [k * 4096, (k + 1) * 4096) of it; a nullable Boolean column with
nulls is one page.  Statistics are compared with what pyarrow's writer records for the same table.
The inputs come from tests/parquet_write_cases.py, which tests/test_parquet_unpage.py checks on the CPU."""
import io

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

import chapterhouseqe_amd as chq
from tests import parquet_unpage as U
from tests import parquet_write_cases as W
from tests.helpers import arrays_identical, batches_identical, explain_diff
from tests.parquet_cases import write_bytes

pytestmark = pytest.mark.gpu

N, PAGE_ROWS = W.N, W.PAGE_ROWS


@pytest.fixture(scope="module")
def ctx():
    c = chq.Context(0)
    c.set_option("parquet_page_rows", PAGE_ROWS)
    yield c
    c.close()


def empty_like(schema: pa.Schema) -> pa.RecordBatch:
    return pa.RecordBatch.from_arrays([pa.array([], type=f.type) for f in schema], schema=schema)


def one_batch(t: pa.Table) -> pa.RecordBatch:
    t = t.combine_chunks()
    return t.to_batches()[0] if t.num_rows else empty_like(t.schema)


def written_twice(write, source, ctx) -> bytes:
    a, b = write(source, ctx=ctx), write(source, ctx=ctx)
    if a != b:
        at = next(k for k in range(min(len(a), len(b))) if a[k] != b[k]) if len(a) == len(b) else -1
        raise AssertionError(f"two images of the same batch differ: {len(a)} and {len(b)} bytes, first at byte {at}")
    return a


def same(got: pa.RecordBatch, want: pa.RecordBatch, who: str):
    assert batches_identical(got, want), f"{who}:\n{explain_diff(got, want)}"


def check_group(raw: bytes, pages, g: int, want: pa.RecordBatch, ctx, mine, bitmap_without_nulls: bool = False):
    """row group g of the image against `want`: pyarrow, the scan, the pages"""
    rows = want.num_rows
    same(one_batch(pq.ParquetFile(io.BytesIO(raw)).read_row_group(g)), want, f"pyarrow, row group {g}")
    same(mine.read_row_group(g, ctx=ctx).to_host(), want, f"the scan, row group {g}")
    same(U.reassemble(raw, pages)[g], want, f"the pages, row group {g}")
    n_pages = max(1, -(-rows // PAGE_ROWS))
    for ci, f in enumerate(want.schema):
        col = want.column(ci)
        ps = [p for p in pages if (p.row_group, p.column) == (g, ci)]
        one_page = pa.types.is_boolean(f.type) and f.nullable and (col.null_count > 0 or (bitmap_without_nulls and len(ps) == 1))
        assert len(ps) == (1 if one_page else n_pages), (f.name, len(ps), n_pages)
        for k, p in enumerate(ps):
            r0 = 0 if one_page else k * PAGE_ROWS
            r1 = rows if one_page else min(rows, (k + 1) * PAGE_ROWS)
            assert p.num_values == r1 - r0, (f.name, k, p.num_values)
            assert arrays_identical(U.page_array(p), col.slice(r0, r1 - r0)), f"{f.name}: page {k} does not hold rows [{r0}, {r1})"
    return [[p for p in pages if (p.row_group, p.column) == (g, ci)] for ci in range(want.num_columns)]


def check_image(raw: bytes, want: pa.RecordBatch, ctx, **kw):
    pages = U.unpage(raw)
    md = pq.ParquetFile(io.BytesIO(raw)).metadata
    assert md.num_row_groups == 1 and md.num_rows == want.num_rows
    mine = chq.ParquetFile(raw)
    try:
        return check_group(raw, pages, 0, want, ctx, mine, **kw)
    finally:
        mine.close()


def both_sources(rec: pa.RecordBatch, ctx):
    return (("host", rec), ("device", chq.DeviceRecordBatch.from_host(rec, ctx=ctx)))


def statistics(raw: bytes, g: int = 0) -> dict:
    md = pq.ParquetFile(io.BytesIO(raw)).metadata.row_group(g)
    return {md.column(i).path_in_schema: md.column(i).statistics for i in range(md.num_columns)}


def same_value(a, b) -> bool:
    return type(a) is type(b) and a == b and (not isinstance(a, float) or np.signbit(a) == np.signbit(b))


def check_statistics(raw: bytes, want: pa.RecordBatch, g: int = 0):
    """the chunk statistics of row group g against those pyarrow's writer records for `want`"""
    got = statistics(raw, g)
    ref = statistics(write_bytes(pa.Table.from_batches([want], schema=want.schema), use_dictionary=False))
    for ci, f in enumerate(want.schema):
        a, b = got[f.name], ref[f.name]
        assert a is not None and a.has_null_count, f.name
        assert a.null_count == b.null_count == want.column(ci).null_count, (f.name, a.null_count, b.null_count)
        assert a.has_min_max == b.has_min_max, (f.name, a.has_min_max, b.has_min_max)
        if b.has_min_max:
            assert same_value(a.min, b.min) and same_value(a.max, b.max), (f.name, a.min, b.min, a.max, b.max)
    return got


# ---- strings ------------------------------------------------------------------------------------------------------------------
def test_string_shapes(ctx):
    """every length 0 .. 145 in sequence (every source and destination alignment of the 16-byte chunks), 255 / 256 / 257,
    4095 / 4096 / 4097, one string of 70 000 bytes (longer than a 256-row step's usual output), nulls before, between and
    after the long strings, the long string under a null, only empty strings, empty strings next to nulls, only nulls; every
    byte depends on its row and its position"""
    rec = one_batch(W.string_shapes())
    assert rec.num_rows == N
    for who, source in both_sources(rec, ctx):
        raw = written_twice(chq.record_to_parquet, source, ctx)
        chunks = check_image(raw, rec, ctx)
        for ci, name in enumerate(rec.schema.names):
            if name in ("empty", "empty_or_null"):      # a valid empty string is its 4-byte length, a null is nothing
                valid = rec.num_rows - rec.column(ci).null_count
                assert sum(p.value_bytes for p in chunks[ci]) == 4 * valid, (who, name)
            if name == "all_null":
                assert all(p.value_bytes == 0 and p.end - p.payload_at == p.level_bytes for p in chunks[ci]), who
        check_statistics(raw, rec)


# ---- validity -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(W.validity_shapes()))
def test_validity_shapes(ctx, shape):
    """runs of nulls and of values aligned with the 64-lane prefix, the 256-row step, the 4096-row block and the page, for
    Int32, Int64, Float32, Float64, Boolean and Utf8 over four pages"""
    valid, nullable, bitmap = W.validity_shapes()[shape]
    rec = W.typed_batch(N, valid, nullable, seed=3, bitmap=bitmap)
    cases = [(who, src, rec, False) for who, src in both_sources(rec, ctx)]
    if bitmap:
        # the bitmap reaches the kernels only where the null count is unknown: a device view of a parent whose nulls lie behind it
        pv = np.ones(N + 8, dtype=bool)
        pv[N:] = False
        parent = W.typed_batch(N + 8, pv, True, seed=4)
        cases.append(("device view", chq.DeviceRecordBatch.from_host(parent, ctx=ctx).slice(0, N), parent.slice(0, N), True))
    for who, source, want, loose in cases:
        raw = written_twice(chq.record_to_parquet, source, ctx)
        chunks = check_image(raw, want, ctx, bitmap_without_nulls=loose)
        st = check_statistics(raw, want)
        for ci, f in enumerate(want.schema):
            ps = chunks[ci]
            if shape == "page1_null" and not pa.types.is_boolean(f.type):
                assert ps[1].value_bytes == 0 and ps[1].end - ps[1].payload_at == ps[1].level_bytes, (who, f.name)
                assert ps[0].value_bytes > 0 and ps[2].value_bytes > 0 and ps[3].value_bytes > 0, (who, f.name)
            if shape == "all_null":
                assert all(p.value_bytes == 0 for p in ps) and not st[f.name].has_min_max and st[f.name].null_count == N, (who, f.name)
            if shape == "nullable_no_buffer":           # one RLE run per page: a length prefix, a varint, the level
                assert all(4 < p.level_bytes <= 4 + 3 for p in ps) and st[f.name].null_count == 0, (who, f.name)
            if shape == "required":
                assert all(p.level_bytes == 0 and not p.optional for p in ps), (who, f.name)
            if shape == "bitmap_all_valid":
                assert st[f.name].null_count == 0 and sum(int(p.levels.sum()) for p in ps) == N, (who, f.name)


# ---- views --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", W.VIEW_OFFSETS)
def test_views_at_chosen_offsets_over_pages(ctx, offset):
    """device and host slices of a larger parent: level bytes shared with the parent (offset a multiple of 8, trailing bits
    of the last byte set) or shifted by pw_shift_bits_kernel, cut into pages; non-null Booleans cut at r0 / 8"""
    for shape in ("random_30", "page1_null"):
        parent = W.view_parent(offset, shape)
        want = parent.slice(offset, N)
        dev = chq.DeviceRecordBatch.from_host(parent, ctx=ctx)
        for who, source in (("device view", dev.slice(offset, N)), ("host view", want)):
            raw = written_twice(chq.record_to_parquet, source, ctx)
            chunks = check_image(raw, want, ctx)
            check_statistics(raw, want)
            if shape == "page1_null":
                for ci, f in enumerate(want.schema):
                    if f.nullable and not pa.types.is_boolean(f.type):
                        assert chunks[ci][1].value_bytes == 0, (who, f.name)


@pytest.mark.parametrize("offset", [8, 9, 4096])
def test_a_view_without_nulls_of_a_parent_with_nulls(ctx, offset):
    """the null count a device view imports is unknown: the chunk must record null_count = 0 and hold every value"""
    parent = W.view_parent(offset, "no_nulls")
    want = parent.slice(offset, N)
    assert all(c.null_count == 0 for c in want.columns) and parent.column(0).null_count > 0
    dev = chq.DeviceRecordBatch.from_host(parent, ctx=ctx)
    for who, source in (("device view", dev.slice(offset, N)), ("host view", want)):
        raw = written_twice(chq.record_to_parquet, source, ctx)
        chunks = check_image(raw, want, ctx, bitmap_without_nulls=True)
        st = check_statistics(raw, want)
        for ci, f in enumerate(want.schema):
            assert st[f.name].null_count == 0 and sum(int(p.levels.sum()) for p in chunks[ci]) == N, (who, f.name)


# ---- several row groups -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nullable", [True, False])
def test_row_groups_with_a_zero_row_batch_between_others(ctx, nullable):
    parts = W.row_group_batches(nullable)
    assert [p.num_rows for p in parts] == [PAGE_ROWS + 1, 0, 1, 2 * PAGE_ROWS]
    device = [chq.DeviceRecordBatch.from_host(p, ctx=ctx) for p in parts]
    for sources in (parts, device, [parts[0], device[1], parts[2], device[3]]):
        raw = written_twice(chq.records_to_parquet, sources, ctx)
        pages = U.unpage(raw)
        md = pq.ParquetFile(io.BytesIO(raw)).metadata
        assert md.num_row_groups == len(parts) and md.num_rows == sum(p.num_rows for p in parts)
        mine = chq.ParquetFile(raw)
        assert mine.num_row_groups == len(parts)
        for g, p in enumerate(parts):
            assert md.row_group(g).num_rows == p.num_rows == mine.row_group_num_rows(g)
            check_group(raw, pages, g, p, ctx, mine)
            if p.num_rows:
                check_statistics(raw, p, g)         # every group's statistics are its own
            else:
                assert all(s is None or (not s.has_min_max and s.null_count == 0) for s in statistics(raw, g).values())
        outs = mine.read_row_groups(ctx=ctx)
        for g, p in enumerate(parts):
            same(outs[g].to_host(), p, f"read_row_groups, row group {g}")
        mine.close()
        same(one_batch(pq.read_table(io.BytesIO(raw))), one_batch(pa.Table.from_batches(parts)), "pyarrow, the whole file")


# ---- statistics ---------------------------------------------------------------------------------------------------------------
def test_statistics_of_sentinels_zeros_nans_and_string_orders(ctx):
    """the reduction's own sentinels (INT64_MAX / INT64_MIN / INT32_MIN as the only value), signed zeros, NaNs of both signs,
    subnormals, infinities, a single value in the last row of the last block, Utf8 ties / prefixes / unsigned byte order /
    minimum and maximum in different blocks of the candidate pass, bounds of 4096 and 4097 bytes; an extreme value lies under
    every null"""
    rec = one_batch(W.statistics_cases())
    for who, source in both_sources(rec, ctx):
        raw = written_twice(chq.record_to_parquet, source, ctx)
        check_image(raw, rec, ctx)
        st = check_statistics(raw, rec)
        # what the issue states outright, whatever pyarrow's writer says
        for k in ("f32_only_pos_zero", "f32_only_neg_zero", "f64_only_pos_zero", "f64_only_neg_zero", "f32_pos_zero_nan", "f64_pos_zero_nan"):
            assert st[k].min == 0 and np.signbit(st[k].min) and st[k].max == 0 and not np.signbit(st[k].max), (who, k)
        for k in ("f32_only_nans_and_nulls", "f64_only_nans_and_nulls", "flag_all_null"):
            assert not st[k].has_min_max and st[k].null_count == rec.column(k).null_count > 0, (who, k)
        for k in ("s_min_4097", "s_max_4097"):
            assert not st[k].has_min_max and st[k].has_null_count and st[k].null_count == 0, (who, k)
        assert st["s_min_4096"].min == W.text(1, 4096) and st["s_max_4096"].max == W.text(1, 4096), who
        for nm, lo, hi in (("i32", -2**31, 2**31 - 1), ("i64", -2**63, 2**63 - 1)):
            assert (st[nm + "_only_min"].min, st[nm + "_only_min"].max) == (lo, lo), who
            assert (st[nm + "_only_max"].min, st[nm + "_only_max"].max) == (hi, hi), who
            assert (st[nm + "_only_max_nulls"].min, st[nm + "_only_min_nulls"].max) == (hi, lo), who
            assert (st[nm + "_min_and_max"].min, st[nm + "_min_and_max"].max) == (lo, hi), who
            assert (st[nm + "_single_value_last_row"].min, st[nm + "_single_value_last_row"].max) == (42, 42), who
        assert (st["f64_zeros_and_subnormals"].min, st["f64_zeros_and_subnormals"].max) == (-5e-324, 5e-324), who
        assert (st["f32_infinities"].min, st["f32_infinities"].max) == (-np.inf, np.inf), who
        assert (st["s_empty_is_min"].min, st["s_shared_prefix"].min, st["s_shared_prefix"].max) == ("", "ab", "abc"), who
        assert (st["s_unsigned_bytes"].min, st["s_unsigned_bytes"].max) == ("A", "\U0001F600"), who
        assert (st["s_min_first_max_last"].min, st["s_min_first_max_last"].max) == ("a", "z"), who
        assert (st["s_max_first_min_last"].min, st["s_max_first_min_last"].max) == ("a", "z"), who
        assert (st["flag_all_false"].max, st["flag_all_true"].min, st["flag_true_under_nulls"].max) == (False, True, False), who


@pytest.mark.parametrize("off", W.STATS_VIEW_OFFSETS)
def test_statistics_of_a_view_are_its_own(ctx, off):
    """the parent holds a smaller and a larger valid value directly before and behind the view, inside the validity bytes the
    view shares with it: a wrong min_value in a footer makes other engines skip row groups"""
    parent = W.statistics_view_parent(off)
    want = parent.slice(off, N)
    dev = chq.DeviceRecordBatch.from_host(parent, ctx=ctx)
    for who, source in (("device view", dev.slice(off, N)), ("host view", want)):
        raw = written_twice(chq.record_to_parquet, source, ctx)
        check_image(raw, want, ctx)
        st = check_statistics(raw, want)
        for k in ("i32", "i64", "req_i64"):
            assert (st[k].min, st[k].max) == (-5, 7), (who, k)
        for k in ("f32", "f64"):
            assert (st[k].min, st[k].max) == (-0.5, 2.5), (who, k)
        for k in ("s", "req_s"):
            assert (st[k].min, st[k].max) == ("g", "p"), (who, k)
        assert (st["flag"].min, st["flag"].max) == (False, False), who
