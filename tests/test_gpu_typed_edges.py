"""GPU: the typed operations of csrc/typed_ops.hip -- Decimal128 comparisons (cmp128_kernel), the Utf8 -> Boolean cast under
AND / OR (utf8_to_bool_kernel) -- and the temporal comparisons that csrc/plan.cpp rewrites to Int32 / Int64 programs, on edge
values, exactly (values, validity, null count, kept rows) against the references of tests/typed_reference.py, which
tests/test_typed_reference.py ties down on the CPU tier.  Neither the oracle nor pyarrow's compute kernels take part.

Where every row runs.  The typed kernels run one thread per row and one ballot per wave, and write one output word per 64
rows; a value test therefore uses a PAIR BATCH (typed_reference.pair_batch_rows): all ordered pairs of the edge table, then
the same pairs rotated by 37 rows, so that every pair sits at two lane positions, in a row count that is no multiple of 64
(Decimal128: 2 * 52^2 = 5 408 rows, 84 complete waves and one of 32 lanes).  The grid-stride second round of these kernels
is tests/test_gpu_rounds.py's.

Which route each test takes (materialize.cpp: fit_subtree -> materialize_typed_op turns a typed operation into a Boolean
temporary column -- bits, validity, null count read back -- before the rest of the expression is lowered):
  * test_decimal128_*: Node::CMP over two T_FIXED_OPAQUE columns -> launch_cmp128.  compute_value and project_record copy the
    temporary out (evaluate_dense); filter_record / filter_project_record / filter_records run the filter kernels over it,
    `x1 < x2 and id > 0` / `x1 = x2 or flag` the accumulator program with the temporary as a Boolean column operand.  Host
    input goes through the staging upload first; a device slice hands the kernel `values + 16 * offset` and the bitmap's bit
    offset.  A batch group with typed operations falls back to one filter_record per batch.
  * test_temporal_*: opaque_compare_class gives Date32 / Time32 the class Int32 and Date64 / Time64 / Timestamp / Duration
    Int64; the typer re-types the two column refs (plan.cpp) and filter.cpp re-types the column itself, so these are
    ordinary programs of the accumulator machine: FU_EQ / FU_LT_I / FU_GT_I (FASTK, tile kinds 0 and 1) for non-null 32-bit
    columns, Interp::compare for nullable ones and at kind 2, the WIDE instantiation for the 64-bit classes.  As in
    tests/test_gpu_int_edges.py the context of these tests forces the large-batch launch structure (`split_rows` = 1) and a
    batch is 16 384 rows repeating the pair table -- complete tiles, the FULL launch -- followed by the pair batch, the
    incomplete tile of the PARTIAL launch.
  * test_utf8_to_boolean_*: Node::TOBOOL over a Utf8 column -> launch_utf8_to_bool (ws_at, parse_bool); `w and flag` is then
    the accumulator's AND over the temporary and `flag`.  test_utf8_to_boolean_trims_exactly_the_white_space_code_points
    walks the whole white-space table of the kernel: every code point of the Basic Multilingual Plane and a sample beyond.

Durations on an MI355X (`pytest --durations=0`, the whole GPU tier in one run; 80 cases, 6.3 s for the module next to 5.9 s
for tests/test_gpu_int_edges.py in the same run): test_temporal_comparisons 4.2 s over its 36 cases, at most 0.25 s a case
(16 546 or 17 184 rows, six operators, up to three tile kinds, compute_value and filter_record each);
test_utf8_to_boolean_on_slices and test_decimal128_comparisons_on_slices at most 0.10 s a case (four windows, six operators
or five forms, device view and host slice); test_utf8_to_boolean_null_slots_enclose_spellings 0.12 s; every other case
below 0.1 s.  The kinds `decimal32`, `decimal64` and `decimal128_edges` of tests/test_gpu_sort.py add 0.4 s to the key-type
tests of the sorted operators, which took 5.0 s without them in that run (join 0.05 s, outer join 0.12 s and 0.13 s for its
new decimal key test, window 0.06 s, aggregate 0.02 s, sort and partition below 0.01 s).
"""
import numpy as np
import pyarrow as pa
import pytest

import chapterhouseqe_amd as chq
from chapterhouseqe_amd.sqlparse import parse_expr, parse_select

from . import typed_reference as R
from .helpers import arrays_identical, batches_identical, explain_diff

pytestmark = pytest.mark.gpu

FULL = 16384
TILE_KINDS = (0, 1, 2)
VIEW_OFFSETS = (1, 7, 63, 64, 65)


@pytest.fixture(scope="module")
def ctx():
    c = chq.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def split_ctx():
    c = chq.Context(0)
    c.set_option("split_rows", 1)
    yield c
    c.close()


def kleene_free(op, a, b):
    """arrow's plain and / or on BooleanArrays: NULL when either side is NULL"""
    if a is None or b is None:
        return None
    return (a and b) if op == "and" else (a or b)


def bools(values):
    return pa.array(list(values), pa.bool_())


def same_bools(got, values, what):
    exp = bools(values)
    if not arrays_identical(got, exp):
        g = got.to_pylist()
        bad = [i for i in range(min(len(g), len(exp))) if g[i] != values[i]]
        raise AssertionError(f"{what}: type {got.type}, length {len(got)} / {len(exp)}, nulls {got.null_count} / {exp.null_count}, "
                             f"{len(bad)} rows differ, first {[(i, g[i], values[i]) for i in bad[:4]]}")


def kept_ids(values):
    return [i for i, v in enumerate(values) if v is True]


def check_kept(got, rec, ids, what):
    """a filter's output: the rows `ids` of `rec`, every column bit for bit"""
    exp = rec.take(pa.array(ids, pa.int64()))
    assert got.column(got.schema.get_field_index("id")).to_pylist() == exp.column(exp.schema.get_field_index("id")).to_pylist(), f"{what}: kept rows differ"
    assert batches_identical(got, exp), f"{what}: {explain_diff(got, exp)}"


# ============================================================================================== Decimal128
PAIRS128 = R.pair_batch_rows(R.I128_EDGES)
N128 = len(PAIRS128)


def null_rows(n, phase):
    """every fifth row from `phase`, and the rows around the wave boundaries"""
    m = np.zeros(n, dtype=bool)
    m[phase::5] = True
    m[[r for r in (0, 63, 64, 65, n - 1) if (r + phase) % 2 == 0]] = True
    return m


def decimal_batch(nulls):
    """x1, x2 over the pair batch, an Int32 row id, a nullable flag.  `nulls`: "none", "left", "right", "both", or "bitmap"
    (both columns carry a validity bitmap without a null)"""
    a, b = [p[0] for p in PAIRS128], [p[1] for p in PAIRS128]
    va = vb = None
    if nulls in ("left", "both"):
        va = ~null_rows(N128, 0)
    if nulls in ("right", "both"):
        vb = ~null_rows(N128, 2)
    if nulls == "bitmap":
        va, vb = np.ones(N128, dtype=bool), np.ones(N128, dtype=bool)
    flag = np.arange(N128) % 3 == 0
    fmask = np.arange(N128) % 7 == 3
    rec = pa.RecordBatch.from_arrays([R.decimal128_array(a, va), R.decimal128_array(b, vb), pa.array(np.arange(N128, dtype=np.int32)),
                                      pa.array(flag, mask=fmask)], names=["x1", "x2", "id", "flag"])
    valid = (np.ones(N128, dtype=bool) if va is None else va) & (np.ones(N128, dtype=bool) if vb is None else vb)
    return rec, valid, [None if m else bool(f) for f, m in zip(flag, fmask)]


def cmp_rows(op, valid, swap=False):
    return [(R.cmp(op, b, a) if swap else R.cmp(op, a, b)) if v else None for (a, b), v in zip(PAIRS128, valid)]


AL4 = [[], [], [], []]
NULLS = ["none", "left", "right", "both", "bitmap"]


@pytest.fixture(scope="module")
def decimal_batches(ctx):
    out = {}
    for nulls in NULLS:
        rec, valid, flag = decimal_batch(nulls)
        out[nulls] = (rec, chq.DeviceRecordBatch.from_host(rec, ctx), valid, flag)
    return out


@pytest.mark.parametrize("nulls", NULLS)
def test_decimal128_comparisons_through_compute_value(ctx, decimal_batches, nulls):
    """six operators, both operand orders, host and device input: values, validity and null count of the Boolean result.  The
    null slots hold every kind of pair, pairs that compare true among them"""
    rec, dev, valid, _ = decimal_batches[nulls]
    if nulls in ("left", "right", "both"):
        assert all(any(R.cmp(op, a, b) for (a, b), v in zip(PAIRS128, valid) if not v) for op in R.CMPS)
    for op in R.CMPS:
        for swap, sql in ((False, f"x1 {op} x2"), (True, f"x2 {op} x1")):
            want = cmp_rows(op, valid, swap)
            for src, name in ((dev, "device"), (rec, "host")):
                got, scalar = chq.compute_value(src, AL4, parse_expr(sql), ctx=ctx)
                assert not scalar
                same_bools(got, want, f"{sql} ({nulls}, {name} input)")


@pytest.mark.parametrize("nulls", NULLS)
def test_decimal128_comparisons_through_filter_record(ctx, decimal_batches, nulls):
    """the kept rows by their row id, the decimal columns of the output by their raw patterns"""
    rec, dev, valid, _ = decimal_batches[nulls]
    for op in R.CMPS:
        for swap, sql in ((False, f"x1 {op} x2"), (True, f"x2 {op} x1")):
            ids = kept_ids(cmp_rows(op, valid, swap))
            check_kept(chq.filter_record(dev, AL4, parse_expr(sql), ctx=ctx).to_host(), rec, ids, f"{sql} ({nulls}, device input)")
            if not swap:
                check_kept(chq.filter_record(rec, AL4, parse_expr(sql), ctx=ctx), rec, ids, f"{sql} ({nulls}, host input)")


@pytest.mark.parametrize("nulls", ["none", "both"])
def test_decimal128_comparisons_through_projection(ctx, decimal_batches, nulls):
    """project_record (`select x1 OP x2 as r, id`) and filter_project_record (`.. where x2 <= x1`), at both `fuse` settings"""
    rec, dev, valid, _ = decimal_batches[nulls]
    keep = kept_ids(cmp_rows("<=", valid, swap=True))
    for op in R.CMPS:
        want = cmp_rows(op, valid)
        sel = parse_select(f"select x1 {op} x2 as r, id from t where x2 <= x1")
        for src, name in ((dev, "device"), (rec, "host")):
            got = chq.project_record(sel.projection, src, AL4, ctx=ctx, device_result=False)
            same_bools(got.column(0), want, f"project x1 {op} x2 ({nulls}, {name} input)")
            assert got.schema.names == ["r", "id"] and got.column(1).to_pylist() == list(range(N128))
        for fuse in (1, 2):
            ctx.set_option("fuse", fuse)
            try:
                got = chq.filter_project_record(sel.selection, sel.projection, dev, AL4, ctx=ctx).to_host()
            finally:
                ctx.set_option("fuse", 1)
            assert got.column(1).to_pylist() == keep, f"filter_project x1 {op} x2 ({nulls}, fuse {fuse}): kept rows differ"
            same_bools(got.column(0), [want[i] for i in keep], f"filter_project x1 {op} x2 ({nulls}, fuse {fuse})")


@pytest.mark.parametrize("nulls", ["none", "both"])
def test_decimal128_comparisons_through_filter_records(ctx, decimal_batches, nulls):
    """the batch cut into five device batches -- one empty, one of one row, cuts inside a wave and inside a validity byte --
    as views of one parent and as uploads of their own"""
    rec, dev, valid, _ = decimal_batches[nulls]
    cuts = [(0, 1001), (1001, 0), (1001, 1), (1002, 3093), (4095, N128 - 4095)]
    assert sum(n for _, n in cuts) == N128
    groups = {"views": [dev.slice(o, n) for o, n in cuts], "uploads": [chq.DeviceRecordBatch.from_host(rec.slice(o, n), ctx) for o, n in cuts]}
    for op in R.CMPS:
        want = cmp_rows(op, valid)
        for name, group in groups.items():
            outs = chq.filter_records(group, AL4, parse_expr(f"x1 {op} x2"), ctx=ctx)
            assert len(outs) == len(cuts)
            for (o, n), out in zip(cuts, outs):
                ids = [o + i for i in kept_ids(want[o:o + n])]
                check_kept(out.to_host(), rec, ids, f"x1 {op} x2 ({nulls}, {name}, batch at {o})")


@pytest.mark.parametrize("offset", VIEW_OFFSETS)
def test_decimal128_comparisons_on_slices(ctx, decimal_batches, offset):
    """device `slice(offset, length)` and host `RecordBatch.slice`: the 16-byte stride and the validity bit offset under an
    offset, lengths that end inside a wave"""
    rec, dev, valid, _ = decimal_batches["both"]
    for length in (1, 100, 1001, N128 - offset - 3):
        assert length % 64 != 0
        views = ((dev.slice(offset, length), "device view"), (rec.slice(offset, length), "host slice"))
        for op in R.CMPS:
            want = cmp_rows(op, valid)[offset:offset + length]
            for src, name in views:
                got, _ = chq.compute_value(src, AL4, parse_expr(f"x1 {op} x2"), ctx=ctx)
                same_bools(got, want, f"x1 {op} x2 ({name} {offset}, {length})")
            ids = [offset + i for i in kept_ids(want)]
            check_kept(chq.filter_record(views[0][0], AL4, parse_expr(f"x2 {op} x1"), ctx=ctx).to_host(), rec,
                       [offset + i for i in kept_ids(cmp_rows(op, valid, swap=True)[offset:offset + length])], f"x2 {op} x1 (device view {offset}, {length})")
            check_kept(chq.filter_record(views[1][0], AL4, parse_expr(f"x1 {op} x2"), ctx=ctx), rec, ids, f"x1 {op} x2 (host slice {offset}, {length})")


@pytest.mark.parametrize("rows", [63, 64, 65])
def test_decimal128_comparisons_row_counts(ctx, decimal_batches, rows):
    """batches that end a row before, at and a row behind the first wave (one row: the slices above): the last wave's validity
    word and null count, for an upload of its own and for a view whose validity is read from a bit offset"""
    rec, dev, valid, _ = decimal_batches["both"]
    sources = ((chq.DeviceRecordBatch.from_host(rec.slice(0, rows), ctx), 0, "upload"), (dev.slice(7, rows), 7, "device view at 7"))
    for op in R.CMPS:
        for src, off, name in sources:
            got, _ = chq.compute_value(src, AL4, parse_expr(f"x1 {op} x2"), ctx=ctx)
            same_bools(got, cmp_rows(op, valid)[off:off + rows], f"x1 {op} x2 ({name}, {rows} rows)")


@pytest.mark.parametrize("nulls", ["none", "left", "both"])
def test_decimal128_comparisons_inside_a_program(ctx, decimal_batches, nulls):
    """the Boolean temporary as an operand of the accumulator machine: `x1 < x2 and id > 0`, `x1 = x2 or flag` (flag nullable;
    AND / OR are not Kleene)"""
    rec, dev, valid, flag = decimal_batches[nulls]
    lt, eq = cmp_rows("<", valid), cmp_rows("=", valid)
    forms = [("x1 < x2 and id > 0", [kleene_free("and", v, i > 0) for i, v in enumerate(lt)]),
             ("id > 0 and x1 < x2", [kleene_free("and", v, i > 0) for i, v in enumerate(lt)]),
             ("x1 = x2 or flag", [kleene_free("or", v, f) for v, f in zip(eq, flag)]),
             ("flag or x2 = x1", [kleene_free("or", v, f) for v, f in zip(eq, flag)])]
    for sql, want in forms:
        for src, name in ((dev, "device"), (rec, "host")):
            got, _ = chq.compute_value(src, AL4, parse_expr(sql), ctx=ctx)
            same_bools(got, want, f"{sql} ({nulls}, {name} input)")
        check_kept(chq.filter_record(dev, AL4, parse_expr(sql), ctx=ctx).to_host(), rec, kept_ids(want), f"{sql} ({nulls})")
    view = dev.slice(65, 1001)
    for sql, want in forms:
        check_kept(chq.filter_record(view, AL4, parse_expr(sql), ctx=ctx).to_host(), rec, [65 + i for i in kept_ids(want[65:65 + 1001])], f"{sql} ({nulls}, view)")


# ============================================================================================== temporal types
TEMPORAL_IDS = [n for n, _ in R.TEMPORAL_TYPES]


def temporal_batch(typ, nullable):
    """FULL rows repeating the pair table (complete tiles), then the pair batch (the incomplete tile)"""
    edges = R.temporal_edges(typ)
    pairs = R.pair_table(edges)
    rows = [pairs[i % len(pairs)] for i in range(FULL)] + R.pair_batch_rows(edges)
    n = len(rows)
    assert n % 64 != 0
    va = vb = None
    if nullable:
        va, vb = ~null_rows(n, 0), np.ones(n, dtype=bool)
        vb[[5, FULL - 1, FULL + 66]] = False
    rec = pa.RecordBatch.from_arrays([R.temporal_array([a for a, _ in rows], typ, va), R.temporal_array([b for _, b in rows], typ, vb),
                                      pa.array(np.arange(n, dtype=np.int32))], names=["x1", "x2", "id"])
    valid = np.ones(n, dtype=bool) if not nullable else va & vb
    return rec, rows, valid


AL3 = [[], [], []]


@pytest.mark.parametrize("nullable", [False, True], ids=["non-null", "nullable"])
@pytest.mark.parametrize("name,typ", R.TEMPORAL_TYPES, ids=TEMPORAL_IDS)
def test_temporal_comparisons(split_ctx, name, typ, nullable):
    """every DataType opaque_compare_class names, all pairs of its edge table, six operators, through compute_value and
    filter_record: tile kinds 0 / 1 / 2 for the 32-bit classes, 2 (WIDE) for the 64-bit ones"""
    ctx = split_ctx
    rec, rows, valid = temporal_batch(typ, nullable)
    dev = chq.DeviceRecordBatch.from_host(rec, ctx)
    try:
        for op in R.CMPS:
            want = [R.cmp(op, a, b) if v else None for (a, b), v in zip(rows, valid)]
            e = parse_expr(f"x1 {op} x2")
            for tk in TILE_KINDS if typ.bit_width == 32 else (2,):
                ctx.set_option("tile_kind", tk)
                got, scalar = chq.compute_value(dev, AL3, e, ctx=ctx)
                assert not scalar
                same_bools(got, want, f"{name}: x1 {op} x2 (tile_kind {tk})")
                check_kept(chq.filter_record(dev, AL3, e, ctx=ctx).to_host(), rec, kept_ids(want), f"{name}: x1 {op} x2 (tile_kind {tk})")
    finally:
        ctx.set_option("tile_kind", 2 if typ.bit_width == 64 else 0)


@pytest.mark.parametrize("name,typ", [("time32_ms", pa.time32("ms")), ("timestamp_ns_utc", pa.timestamp("ns", tz="UTC"))], ids=["32-bit", "64-bit"])
def test_temporal_comparisons_nested_in_the_other_entry_points(split_ctx, name, typ):
    """`(x1 < x2 or x1 = x2) and id >= 0` and a projected comparison through filter_project_record (both `fuse` settings),
    and the predicate through filter_records over five device batches, one empty and one of one row"""
    ctx = split_ctx
    rec, rows, valid = temporal_batch(typ, True)
    n = len(rows)
    dev = chq.DeviceRecordBatch.from_host(rec, ctx)
    le = [R.cmp("<=", a, b) if v else None for (a, b), v in zip(rows, valid)]
    ne = [R.cmp("<>", a, b) if v else None for (a, b), v in zip(rows, valid)]
    sel = parse_select("select x2 <> x1 as r, id from t where (x1 < x2 or x1 = x2) and id >= 0")
    keep = kept_ids(le)
    for fuse in (1, 2):
        ctx.set_option("fuse", fuse)
        try:
            got = chq.filter_project_record(sel.selection, sel.projection, dev, AL3, ctx=ctx).to_host()
        finally:
            ctx.set_option("fuse", 1)
        assert got.column(1).to_pylist() == keep, f"{name} (fuse {fuse}): kept rows differ"
        same_bools(got.column(0), [ne[i] for i in keep], f"{name} (fuse {fuse})")
    cuts = [(0, 1001), (1001, 0), (1001, 1), (1002, FULL - 1002 + 37), (FULL + 37, n - FULL - 37)]
    assert sum(c for _, c in cuts) == n
    outs = chq.filter_records([dev.slice(o, c) for o, c in cuts], AL3, sel.selection, ctx=ctx)
    for (o, c), out in zip(cuts, outs):
        check_kept(out.to_host(), rec, [o + i for i in kept_ids(le[o:o + c])], f"{name}: batch at {o}")


# ============================================================================================== Utf8 -> Boolean
WORDS = R.BOOL_WORDS
CAST = [e for _, e in R.BOOL_WORD_TABLE]
NW = len(WORDS)


def words_batch(words, valid=None, trailing=b""):
    """w, an all-true t, an all-false f, a nullable flag, a row id"""
    n = len(words)
    flag, fmask = np.arange(n) % 2 == 0, np.arange(n) % 5 == 1
    rec = pa.RecordBatch.from_arrays([R.utf8_array(words, valid, trailing), pa.array(np.ones(n, dtype=bool)), pa.array(np.zeros(n, dtype=bool)),
                                      pa.array(flag, mask=fmask), pa.array(np.arange(n, dtype=np.int32))], names=["w", "t", "f", "flag", "id"])
    return rec, [None if m else bool(f) for f, m in zip(flag, fmask)]


AL5 = [[], [], [], [], []]


def word_forms(cast, flag):
    """(sql, expected) of the four forms over a batch whose word column casts to `cast`"""
    return [("w and t", list(cast)), ("w or f", list(cast)), ("w and flag", [kleene_free("and", c, f) for c, f in zip(cast, flag)]),
            ("w or flag", [kleene_free("or", c, f) for c, f in zip(cast, flag)]), ("flag and w", [kleene_free("and", c, f) for c, f in zip(cast, flag)])]


def check_words(ctx, src, rec, cast, flag, what, base=0):
    """the four forms through compute_value, filter_record and project_record.  `rec`: the host batch the row ids index,
    `base`: the id of the first row of `src`"""
    dev_in = isinstance(src, chq.DeviceRecordBatch)
    for sql, want in word_forms(cast, flag):
        got, scalar = chq.compute_value(src, AL5, parse_expr(sql), ctx=ctx)
        assert not scalar
        same_bools(got, want, f"{sql} ({what})")
        out = chq.filter_record(src, AL5, parse_expr(sql), ctx=ctx)
        check_kept(out.to_host() if dev_in else out, rec, [base + i for i in kept_ids(want)], f"{sql} ({what})")
    sel = parse_select("select w and flag as r, id, w or f as c from t")
    got = chq.project_record(sel.projection, src, AL5, ctx=ctx, device_result=False)
    forms = dict(word_forms(cast, flag))
    same_bools(got.column(0), forms["w and flag"], f"project w and flag ({what})")
    same_bools(got.column(2), forms["w or f"], f"project w or f ({what})")
    assert got.column(1).to_pylist() == list(range(base, base + len(cast)))


def test_utf8_to_boolean_word_table(ctx):
    """the whole table as one column, host and device input"""
    rec, flag = words_batch(WORDS)
    check_words(ctx, chq.DeviceRecordBatch.from_host(rec, ctx), rec, CAST, flag, "table, device input")
    check_words(ctx, rec, rec, CAST, flag, "table, host input")


@pytest.mark.parametrize("rows", [1, 63, 64, 65])
def test_utf8_to_boolean_row_counts(ctx, rows):
    """one lane, a wave short of one lane, a whole wave, a wave and one lane: rows spread over the table"""
    idx = [(7 + 29 * i) % NW for i in range(rows)]
    assert len({CAST[i] for i in idx}) == (3 if rows > 1 else 1)
    rec, flag = words_batch([WORDS[i] for i in idx])
    check_words(ctx, chq.DeviceRecordBatch.from_host(rec, ctx), rec, [CAST[i] for i in idx], flag, f"{rows} rows")


def test_utf8_to_boolean_null_slots_enclose_spellings(ctx):
    """a nullable word column: every null slot encloses bytes (`true` among them) and must come out NULL; the last row is
    null over a non-empty extent at the very end of the data buffer, and bytes nobody owns follow it"""
    valid = np.arange(NW) % 3 != 1
    words = list(WORDS)
    for i in range(1, NW, 6):
        words[i] = b"true"
    words[-1], valid[-1] = b" TRUE ", False
    assert all(len(words[i]) > 0 for i in range(NW) if not valid[i] and i % 6 == 1) and sum(1 for i in range(NW) if not valid[i] and words[i] == b"true") > 100
    cast = [R.utf8_to_bool(w) if v else None for w, v in zip(words, valid)]
    for trailing in (b"", b"1"):
        rec, flag = words_batch(words, valid, trailing)
        check_words(ctx, chq.DeviceRecordBatch.from_host(rec, ctx), rec, cast, flag, f"nullable words, {len(trailing)} trailing bytes")
    check_words(ctx, rec, rec, cast, flag, "nullable words, host input")


def test_utf8_to_boolean_nul_bytes_behind_a_spelling(ctx):
    """`true\\0`, `0\\0`, `f\\0\\0\\0\\0`: NULL.  (parse_bool packs the trimmed bytes into one integer that does not hold their
    number; before it refused NUL bytes, a spelling followed by NUL bytes had the spelling's key and came out true / false.
    Found by the word table's `true\\0` rows)"""
    words = [s + b"\x00" * k for s in R.TRUE_SPELLINGS + R.FALSE_SPELLINGS for k in range(1, 6 - len(s))]
    words += [b"true\x00 ", b" 0\x00", b"\x00", b"\x00\x00\x00\x00\x00", b"TRUE\x00", b"\xe2\x80\x83no\x00\xe2\x80\x83"]
    assert b"true\x00" in words and b"0\x00" in words and all(R.utf8_to_bool(w) is None for w in words)
    rec, flag = words_batch(words)
    check_words(ctx, chq.DeviceRecordBatch.from_host(rec, ctx), rec, [None] * len(words), flag, "NUL bytes behind a spelling")


@pytest.mark.parametrize("offset", VIEW_OFFSETS)
def test_utf8_to_boolean_on_slices(ctx, offset):
    """device views and host slices of a nullable word column: offsets[0] != 0, the validity bit offset, lengths that end
    inside a wave"""
    valid = np.arange(NW) % 4 != 2
    rec, flag = words_batch(WORDS, valid)
    dev = chq.DeviceRecordBatch.from_host(rec, ctx)
    cast = [c if v else None for c, v in zip(CAST, valid)]
    for length in (1, 100, 1001, NW - offset - 3):
        assert length % 64 != 0
        sl = slice(offset, offset + length)
        check_words(ctx, dev.slice(offset, length), rec, cast[sl], flag[sl], f"device view ({offset}, {length})", base=offset)
        check_words(ctx, rec.slice(offset, length), rec, cast[sl], flag[sl], f"host slice ({offset}, {length})", base=offset)


def test_utf8_to_boolean_through_filter_records(ctx):
    """five device batches, one empty and one of one row, as views of one parent and as uploads of their own"""
    valid = np.arange(NW) % 4 != 2
    rec, flag = words_batch(WORDS, valid)
    dev = chq.DeviceRecordBatch.from_host(rec, ctx)
    cast = [c if v else None for c, v in zip(CAST, valid)]
    cuts = [(0, 129), (129, 0), (129, 1), (130, 1001), (1131, NW - 1131)]
    assert sum(n for _, n in cuts) == NW
    groups = {"views": [dev.slice(o, n) for o, n in cuts], "uploads": [chq.DeviceRecordBatch.from_host(rec.slice(o, n), ctx) for o, n in cuts]}
    for sql, want in word_forms(cast, flag):
        for name, group in groups.items():
            outs = chq.filter_records(group, AL5, parse_expr(sql), ctx=ctx)
            for (o, n), out in zip(cuts, outs):
                check_kept(out.to_host(), rec, [o + i for i in kept_ids(want[o:o + n])], f"{sql} ({name}, batch at {o})")


@pytest.mark.parametrize("nulls", [False, True], ids=["non-null", "nullable"])
@pytest.mark.parametrize("rows", [1, 64, 100])
def test_utf8_to_boolean_all_empty_column_without_a_data_buffer(ctx, rows, nulls):
    """a caller-owned Utf8 column whose offsets are all zero and whose data pointer is null: every row casts to NULL"""
    valid = np.arange(rows + 1) % 3 != 1
    up = chq.DeviceRecordBatch.from_host(pa.RecordBatch.from_arrays(
        [pa.array(np.zeros(rows + 1, np.int32)), pa.array(np.ones(rows + 1, dtype=bool)), pa.array(valid)], names=["o", "t", "v"]), ctx)
    w = {"name": "w", "format": "u", "values": up.column_buffer_address(0)}
    if nulls:
        w.update(validity=up.column_buffer_address(2), null_count=int((~valid[:rows]).sum()), nullable=True)
    dev = chq.DeviceRecordBatch.from_device_buffers([w, {"name": "t", "format": "b", "values": up.column_buffer_address(1)}], rows, ctx, keepalive=[up])
    assert dev.column_buffer_address(0, 2) == 0
    for sql in ("w and t", "w or t", "t and w"):
        got, _ = chq.compute_value(dev, [[], []], parse_expr(sql), ctx=ctx)
        same_bools(got, [None] * rows, f"{sql} ({rows} rows)")
        assert chq.filter_record(dev, [[], []], parse_expr(sql), ctx=ctx).num_rows == 0
    host = pa.RecordBatch.from_arrays([pa.array([""] * rows, pa.utf8()), pa.array(np.ones(rows, dtype=bool))], names=["w", "t"])
    got, _ = chq.compute_value(host, [[], []], parse_expr("w and t"), ctx=ctx)
    same_bools(got, [None] * rows, f"host column of empty strings ({rows} rows)")


def test_utf8_to_boolean_trims_exactly_the_white_space_code_points(ctx):
    """`c 1 c` for every code point c of the Basic Multilingual Plane and every 257th beyond it: true exactly for the 25
    members of White_Space, NULL for everything else -- the kernel's whole table, and nothing a table could name by mistake"""
    cps = [c for c in range(0x10000) if not 0xD800 <= c <= 0xDFFF] + list(range(0x10000, 0x110000, 257))
    words = [chr(c).encode("utf-8") + b"1" + chr(c).encode("utf-8") for c in cps]
    rec = pa.RecordBatch.from_arrays([R.utf8_array(words), pa.array(np.ones(len(cps), dtype=bool))], names=["w", "t"])
    got, _ = chq.compute_value(rec, [[], []], parse_expr("w and t"), ctx=ctx)
    ws = set(R.WHITE_SPACE)
    trimmed = {c for c, v in zip(cps, got.to_pylist()) if v is not None}
    assert trimmed == ws, sorted(hex(c) for c in trimmed ^ ws)
    same_bools(got, [True if c in ws else None for c in cps], "c 1 c")
