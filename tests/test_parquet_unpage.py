"""The page reader of the encoder tests (tests/parquet_unpage.py) checked against pyarrow, no GPU and no libchq: on files
pyarrow writes PLAIN / V1 / uncompressed in many small pages, the pages put together again are pyarrow's own read of the same
bytes -- all six types, with and without nulls, 0, 1 and several thousand rows, one and several row groups -- and a file
that breaks one of the rules the reader asserts is refused.  The shape builders of tests/parquet_write_cases.py, which the GPU
suite shares, are checked for the properties their names promise."""
import io

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

from tests import parquet_forge as P
from tests import parquet_unpage as U
from tests import parquet_write_cases as W
from tests.helpers import batches_identical, explain_diff
from tests.snappy_forge import footer, rewrite, thrift_bytes

PLAIN_V1 = dict(use_dictionary=False, compression="none", data_page_version="1.0", data_page_size=300, write_batch_size=64)


def pa_write(t, **kw) -> bytes:
    buf = io.BytesIO()
    pq.write_table(t, buf, **{**PLAIN_V1, **kw})
    return buf.getvalue()


def as_table(rec: pa.RecordBatch) -> pa.Table:
    return pa.Table.from_batches([rec], schema=rec.schema)


def check_against_pyarrow(raw: bytes, min_pages: int = 1):
    pages = U.unpage(raw)
    got = U.reassemble(raw, pages)
    f = pq.ParquetFile(io.BytesIO(raw))
    assert len(got) == f.metadata.num_row_groups
    for g, rec in enumerate(got):
        want = f.read_row_group(g).combine_chunks()
        want = want.to_batches()[0] if want.num_rows else pa.RecordBatch.from_arrays([pa.array([], type=x.type) for x in want.schema], schema=want.schema)
        assert batches_identical(rec, want), explain_diff(rec, want)
        for ci in range(rec.num_columns):
            mine = [p for p in pages if (p.row_group, p.column) == (g, ci)]
            few = pa.types.is_boolean(rec.schema.field(ci).type)      # (bits: an eighth of the bytes)
            assert len(mine) >= (min(min_pages, 2 if few else min_pages) if rec.num_rows else 0), (g, ci, len(mine))
            assert [p.page for p in mine] == list(range(len(mine)))
            nulls = sum(int(p.num_values - p.levels.sum()) for p in mine)
            assert nulls == want.column(ci).null_count
    return pages


@pytest.mark.parametrize("n", [0, 1, W.N])
@pytest.mark.parametrize("shape", ["random_30", "page1_null", "all_null", "only_last_row", "nullable_no_buffer", "required"])
def test_pages_put_together_are_pyarrows_read(n, shape):
    valid, nullable, bitmap = W.validity_shapes(max(n, 1))[shape]
    rec = W.typed_batch(n, None if valid is None else valid[:n], nullable, seed=n, bitmap=bitmap)
    raw = pa_write(as_table(rec))
    pages = check_against_pyarrow(raw, min_pages=4 if n == W.N and shape not in ("all_null", "only_last_row") else 1)
    back = U.reassemble(raw, pages)[0]
    assert batches_identical(back, rec), explain_diff(back, rec)     # (and the input itself, NaN payloads included)


def test_several_row_groups_and_the_shared_tables():
    for t in (W.string_shapes(), W.statistics_cases(), as_table(W.view_parent(9, "page1_null"))):
        check_against_pyarrow(pa_write(t, data_page_size=20_000, write_batch_size=256))
    pages = check_against_pyarrow(pa_write(as_table(W.typed_batch(W.N, W.thirty_percent(W.N))), row_group_size=5000))
    assert {p.row_group for p in pages} == {0, 1, 2}
    parts = W.row_group_batches(True)
    assert [p.num_rows for p in parts] == list(W.ROW_GROUP_ROWS)


def test_the_reader_recovers_the_null_count_through_sections_and_decode():
    rec = W.typed_batch(W.N, W.thirty_percent(W.N))
    raw = pa_write(as_table(rec))
    nulls = 0
    for sec in P.sections(raw):
        if sec.info.column == 0:
            lv, _ = P.decode(sec.levels, 1, sec.info.num_values)
            nulls += int(sec.info.num_values - lv.sum())
    assert nulls == rec.column(0).null_count > 0


# ---- a file that breaks a rule is refused ------------------------------------------------------------------------------------
def small_file() -> bytes:
    n = 700
    valid = W.thirty_percent(n)
    return pa_write(as_table(W.typed_batch(n, valid)), data_page_size=400)


def edit_footer(raw: bytes, fn) -> bytes:
    meta = footer(raw)
    fn(meta)
    foot = thrift_bytes(meta)
    n = int.from_bytes(raw[-8:-4], "little")
    return raw[:len(raw) - 8 - n] + foot + len(foot).to_bytes(4, "little") + b"PAR1"


def chunk(meta, ci, gi=0):
    return meta.get(4)[1][gi].get(1)[1][ci].get(3)


def on_page(column: int, page: int, fn):
    """a parquet_forge.repack callback that hands one page's (levels, values) to fn"""
    return lambda sec: fn(sec.levels, sec.values) if (sec.info.column, sec.info.page) == (column, page) else None


def header_edit(column: int, page: int, fn):
    def page_fn(info, payload):
        if (info.column, info.page) == (column, page):
            fn(info.header)
        return None
    return page_fn


S = list(W.TYPES).index("s")
FLAG = list(W.TYPES).index("flag")


def flip_first_null(levels: bytes, values: bytes):
    """one more set level bit than the page has values (the levels of these small pages: bit-packed runs)"""
    lv = bytearray(levels)
    assert lv[0] & 1, "a bit-packed run first"
    for k in range(1, len(lv)):
        if lv[k] != 0xFF:
            lv[k] |= lv[k] + 1
            return bytes(lv), None
    raise AssertionError("no null in this page")


BROKEN = {
    "a value byte too few": lambda raw: P.repack(raw, on_page(0, 1, lambda lv, vs: (None, vs[:-1]))),
    "a value byte left over": lambda raw: P.repack(raw, on_page(2, 0, lambda lv, vs: (None, vs + b"\0"))),
    "a Boolean byte left over": lambda raw: P.repack(raw, on_page(FLAG, 0, lambda lv, vs: (None, vs + b"\0"))),
    "a string that ends behind its page": lambda raw: P.repack(raw, on_page(S, 1, lambda lv, vs: (None, (int.from_bytes(vs[:4], "little") + 1).to_bytes(4, "little") + vs[4:]))),
    "a last string cut short": lambda raw: P.repack(raw, on_page(S, 1, lambda lv, vs: (None, vs[:-1]))),
    "more level bits than values": lambda raw: P.repack(raw, on_page(1, 1, flip_first_null)),
    "level bytes left over": lambda raw: P.repack(raw, on_page(1, 0, lambda lv, vs: (lv + b"\0", None))),
    "levels that end before num_values": lambda raw: rewrite(raw, header_edit(3, 1, lambda ph: ph.get(5).set(1, ph.get(5).get(1) + 4000)), None),
    "uncompressed size unlike the payload": lambda raw: rewrite(raw, header_edit(0, 0, lambda ph: ph.set(2, ph.get(2) + 1)), None),
    "a page with a value too many": lambda raw: rewrite(raw, header_edit(1, 1, lambda ph: ph.get(5).set(1, ph.get(5).get(1) + 1)), None),
    "a chunk that starts a byte late": lambda raw: edit_footer(raw, lambda m: chunk(m, 2).set(9, chunk(m, 2).get(9) + 1)),
    "a chunk that ends a byte early": lambda raw: edit_footer(raw, lambda m: chunk(m, 5).set(7, chunk(m, 5).get(7) - 1)),
    "a last chunk that stops before the footer": lambda raw: raw[:len(raw) - 8 - int.from_bytes(raw[-8:-4], "little")] + b"\0" + raw[len(raw) - 8 - int.from_bytes(raw[-8:-4], "little"):],
    "a row group with a row more": lambda raw: edit_footer(raw, lambda m: m.get(4)[1][0].set(3, m.get(4)[1][0].get(3) + 1)),
}


@pytest.mark.parametrize("name", list(BROKEN))
def test_a_file_that_breaks_a_rule_is_refused(name):
    raw = small_file()
    assert len(U.unpage(raw)) >= 12
    bad = BROKEN[name](raw)
    assert bad != raw
    with pytest.raises(U.UnpageError):
        U.unpage(bad)


def test_a_level_length_prefix_that_points_behind_the_payload_is_refused():
    raw = small_file()
    pg = [p for p in U.unpage(raw) if (p.column, p.page) == (1, 1)][0]
    bad = bytearray(raw)
    bad[pg.payload_at:pg.payload_at + 4] = (pg.end - pg.payload_at).to_bytes(4, "little")
    with pytest.raises(U.UnpageError):
        U.unpage(bytes(bad))


# ---- the shape builders -------------------------------------------------------------------------------------------------------
def test_string_bytes_depend_on_row_and_position():
    offs, data = W.text_bytes([5], [70_000])
    chunks = {data[k:k + 16].tobytes() for k in range(0, 70_000 - 15, 16)}
    assert len(chunks) == 70_000 // 16                               # no two 16-byte chunks of one string are equal
    assert set(data.tolist()) == set(range(0x20, 0x7F))
    a, b = W.text_bytes([5], [300])[1], W.text_bytes([6], [300])[1]
    assert (a != b).all()                                            # neighbouring rows differ everywhere
    assert all(len({W.text(r, ln)[k:k + 16] for k in range(0, ln - 15, 16)}) == ln // 16 for r in (0, 1, 77) for ln in (145, 257, 4097))
    t = W.string_shapes()
    assert t.num_rows == W.N and t.column("ladder").null_count == 0 and t.column("all_null").null_count == W.N
    lens = pa.compute.utf8_length(t.column("ladder")).to_pylist()
    assert lens[:len(W.STRING_LENGTHS)] == W.STRING_LENGTHS and lens[W.LONG_AT + 6] == 70_000
    # every source and destination alignment of the 16-byte chunks occurs among the ladder's rows of 16 bytes or more
    src = np.cumsum([0] + lens[:-1])
    dst = np.cumsum([0] + [4 + x for x in lens[:-1]]) + 4
    long = np.array(lens) >= 16
    assert set((src[long] % 16).tolist()) == set(range(16)) and set((dst[long] % 16).tolist()) == set(range(16))
    for name in ("ladder_nulls", "ladder_long_under_null"):
        v = np.asarray(t.column(name).combine_chunks().is_valid())
        assert not v[W.LONG_AT - 1] or name != "ladder_nulls"
        assert v[W.LONG_AT + 6] == (name == "ladder_nulls") and 0 < t.column(name).null_count < W.N
    e = t.column("empty_or_null").combine_chunks()
    assert e.null_count == (W.N + 1) // 3 and set(e.to_pylist()) == {"", None}


def test_validity_shapes_are_what_their_names_say():
    shapes = W.validity_shapes()
    assert len(shapes) == 12
    n, pr = W.N, W.PAGE_ROWS
    assert n == 3 * pr + 5
    v = {k: s[0] for k, s in shapes.items()}
    assert v["bitmap_all_valid"].all() and shapes["bitmap_all_valid"][2] and not v["all_null"].any()
    assert np.flatnonzero(v["only_row_0"]).tolist() == [0] and np.flatnonzero(v["only_last_row"]).tolist() == [n - 1]
    assert np.flatnonzero(v["edge_rows"]).tolist() == [63, 64, 255, 256, 4095, 4096, n - 1]
    assert (v["all_but_edge_rows"] != v["edge_rows"]).all()
    assert not v["block0_null_block1_valid"][:pr].any() and v["block0_null_block1_valid"][pr:2 * pr].all()
    assert v["block0_valid_block1_null"][:pr].all() and not v["block0_valid_block1_null"][pr:2 * pr].any()
    p1 = v["page1_null"]
    assert not p1[pr:2 * pr].any() and p1[pr - 1] and p1[2 * pr] and p1[:pr].any() and p1[2 * pr:].any()
    assert 0.25 < 1 - v["random_30"].mean() < 0.35
    assert v["nullable_no_buffer"] is None and shapes["nullable_no_buffer"][1] and not shapes["required"][1]
    rec = W.typed_batch(n, v["bitmap_all_valid"], bitmap=True)
    assert all(c.null_count == 0 and c.buffers()[0] is not None for c in rec.columns)
    for off in W.VIEW_OFFSETS:
        par = W.view_parent(off, "random_30")
        assert par.num_rows == W.VIEW_PARENT_ROWS
        valid = np.asarray(par.column(0).is_valid())
        assert valid[off + n:off + n + 8].all() and not valid[off + n + 8:off + n + 16].any()
        assert par.slice(off, n).column("s").null_count == par.slice(off, n).column("i32").null_count > 0
    par = W.view_parent(9, "no_nulls")
    assert par.column("f64").null_count > 0 and par.slice(9, n).column("f64").null_count == 0


def test_statistics_cases_hold_what_the_issue_lists():
    t = W.statistics_cases()
    assert t.num_rows == W.N and t.num_columns >= 50
    c = lambda k: t.column(k).combine_chunks()
    assert set(c("i64_only_min").to_pylist()) == {-2**63} and set(c("i32_only_max").to_pylist()) == {2**31 - 1}
    assert set(c("i64_only_max_nulls").to_pylist()) == {2**63 - 1, None}
    assert c("i32_single_value_last_row").to_pylist()[-1] == 42 and c("i32_single_value_last_row").null_count == W.N - 1
    assert np.signbit(c("f64_only_neg_zero").to_numpy()).all() and not np.signbit(c("f32_only_pos_zero").to_numpy()).any()
    z = c("f64_zeros_and_subnormals").to_numpy()
    assert set(z.view(np.uint64).tolist()) == {0, 1 << 63, 1, (1 << 63) | 1}
    nn = c("f32_only_nans_and_nulls")
    assert nn.null_count > 0 and np.isnan(nn.drop_null().to_numpy()).all() and np.signbit(nn.drop_null().to_numpy()).any()
    assert len(c("s_min_4097")[0].as_py()) == 4097 and len(c("s_max_4096")[0].as_py()) == 4096
    # what pyarrow's writer records for them (the values the issue states)
    md = pq.ParquetFile(io.BytesIO(pa_write(t, data_page_size=1 << 20))).metadata.row_group(0)
    st = {md.column(i).path_in_schema: md.column(i).statistics for i in range(md.num_columns)}
    for k in ("f32_only_pos_zero", "f32_only_neg_zero", "f64_only_pos_zero", "f64_only_neg_zero"):
        assert st[k].has_min_max and np.signbit(st[k].min) and st[k].max == 0 and not np.signbit(st[k].max), k
    for k in ("f32_only_nans_and_nulls", "f64_only_nans_and_nulls", "flag_all_null"):
        assert not st[k].has_min_max and st[k].null_count == c(k).null_count > 0, k
    for k in ("s_min_4097", "s_max_4097"):
        assert not st[k].has_min_max and st[k].null_count == 0, k
    for k in ("s_min_4096", "s_max_4096"):
        assert st[k].has_min_max and 4096 in (len(st[k].min), len(st[k].max)), k
    assert st["s_unsigned_bytes"].min == "A" and st["s_unsigned_bytes"].max == "\U0001F600"
    assert st["s_shared_prefix"].min == "ab" and st["s_shared_prefix"].max == "abc"
    assert st["s_min_under_null"].min == "m" and st["s_min_under_null"].max == "\x7f"
    for off in W.STATS_VIEW_OFFSETS:
        assert (off + W.N) // 8 == (off + W.N - 1) // 8 and W.statistics_view_parent(off).column("i32").is_valid()[off + W.N].as_py()
    assert (5 - 1) // 8 == 5 // 8
    par = W.statistics_view_parent(5)
    view = par.slice(5, W.N)
    assert pa.compute.min(par.column("i32")).as_py() == -2**31 and pa.compute.min(view.column("i32")).as_py() == -5
    assert pa.compute.max(par.column("s")).as_py() == "zzzz" and pa.compute.max(view.column("s")).as_py() == "p"
    assert pa.compute.max(view.column("flag")).as_py() is False and pa.compute.max(par.column("flag")).as_py() is True
