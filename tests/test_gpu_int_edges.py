"""GPU: checked integer arithmetic, comparisons, widening and integer -> Boolean on range-edge values, exactly (values,
result types, status codes and the reported row) against the reference of tests/int_reference.py -- the tables
tests/test_int_reference.py ties to pyarrow's checked kernels and to the oracle on the CPU tier.

Where every row runs.  As in tests/test_gpu_float_edges.py the context forces the large-batch launch structure
(`split_rows` = 1: complete tiles in the FULL-only instantiation, the incomplete last tile in a PARTIAL launch) and a value
batch is 16 384 rows repeating a table -- one complete tile of `tile_kind` 0, eight of kinds 1 and 2 -- followed by a chunk of
at most 1 500 rows, the incomplete tile.  The chunks walk the whole table (every table here fits one chunk), so every row
is evaluated in a complete tile of the FULL launch and in the incomplete tile of the PARTIAL launch.  A wave covers 1 024
rows at kind 0 (BLOCK 1024, R 16) and 512 at kinds 1 and 2 (BLOCK 256, R 8); lane l, slot j holds row w0 + 64 j + l.

Which instantiation runs (filter.cpp: encode_fast_uops, pick_tile_kind; kernels.hip: launch_filter / launch_project /
launch_filter_project) is decided by construction -- `last_stats` does not report it:
  * "i32-fast": tile kinds 0 and 1, FASTK (run_fast): programs whose every instruction works on non-null Int32 / UInt32
    columns and Int32 literals -- `+ - *` (FU_ADD_I .. FU_MUL_U), `/` and `%` by a literal 2^k, k <= 30, on the right
    (FU_DIVP2_I / FU_REMP2_I), the six comparisons (FU_EQ, FU_LT_I / FU_GT_I / FU_LT_U / FU_GT_U, FU_NEGATE).  run_fast also
    evaluates the incomplete waves of the PARTIAL tile.  A lone `column <cmp> literal` -- nullable or not -- takes
    run_cmp_const in complete waves and run_fast in incomplete ones.  With `tile_kind` 2 the same programs run in the
    generic interpreter.
  * "generic": tile kinds 0 / 1 / 2, Interp::arith / compare / convert with WIDE = false: the same programs when a column
    has a validity bitmap with nulls, every general `/` and `%` (one such instruction sends the whole program here), and
    every program over an Int8 / Int16 / UInt8 / UInt16 column.  Int8 .. UInt16 compute in the 32-bit class and are
    range-checked against their own type.
  * "wide": any Int64 / UInt64 operand, or a numeric temporary (`(p / z) + (x * y)`): kind 2 (WIDE = true) whatever the
    `tile_kind` option says.
  * filter_project_kernel (`fuse` = 2) is one launch with no FULL / PARTIAL split: kinds 0 and 1 for Int32 / UInt32, kind 2
    for Int64 / UInt64.  When it flags an error the host discards its result and runs filter_record, then project_record
    on the survivors: the row a projection error reports is the row of project_record's input.
How literals lower (plan.cpp; `describe_plan` prints it): `x OP c` is LOAD x; OP const.  `c OP x` is LOAD const; OP x -- a
column operand, NOT a reversed instruction -- so `8 / x` is a real division in the generic interpreter.  The reversed
literal forms (IF_REV: FU_RSUB_I, and Interp::arith's `!rev` guard of the 2^k shortcut) are reached by `c OP (x + 0)`;
reversed column operands (FU_RSUB_U) by `x - (y * one)`.  Negative constants are folded `(0 - c)` under `enable_minus`.

Not reachable from SQL, and therefore not covered here: an integer literal is Int32 (Int64 when it does not fit) and
UInt32 with Int32 / Int64-literal is a coercion miss (`u32 + 1`: status 9), UInt8 / UInt16 with a literal compute as Int32.
So no UInt32 instruction ever has a literal operand: FU_DIVP2_U and FU_REMP2_U altogether, FU_ADD_U / FU_SUB_U / FU_RSUB_U /
FU_MUL_U / FU_LT_U / FU_GT_U with FO_CONST, run_cmp_const's T_U32 arm, and the C_U32 arm of Interp::arith's 2^k shortcut
and of Interp::compare's literal branch.  The UInt32 forms with column operands are covered.

Durations on an MI355X (`pytest --durations=0`; 292 cases, 7.6 s for the module): test_comparisons_against_literals 0.99 s
(generic) and 0.97 s (fast) -- 108 forms through filter_record and 72 through compute_value at three tile kinds;
test_arithmetic_through_compute_value[i32-fast-+] 0.50 s (the first case: it loads the library and creates the context);
test_reported_row_at_wave_tile_and_launch_boundaries at most 0.13 s (204 uploaded batches, 612 failing calls);
test_every_failing_pair_is_detected at most 0.08 s (signed `*`: 851 / 859 uploads and launches of at most 1 500 rows, about
90 microseconds each); every other case below 0.1 s.
"""
import re

import numpy as np
import pyarrow as pa
import pytest

import chapterhouseqe_amd as chq
from chapterhouseqe_amd.sqlparse import parse_expr, parse_select
from oracle import oracle as O

from . import int_reference as R
from .helpers import arrays_identical, batches_identical, explain_diff

pytestmark = pytest.mark.gpu

FULL, CHUNK = 16384, 1500
TILE_KINDS = (0, 1, 2)
NULL_ROWS = (5, 4096 + 77, 2 * 4096 + 1031, 3 * 4096 + 4000)
WAVE_ROWS = {0: 1024, 1: 512, 2: 512}
TILE_ROWS = {0: 16384, 1: 2048, 2: 2048}
TYPE_OPS = [(t, op) for t in R.TYPES for op in R.OPS]
TYPE_OP_IDS = [f"{t}{op}" for t, op in TYPE_OPS]
# (type, evaluator): the cells of the matrix above
CELLS = [("i32", "fast"), ("i32", "generic"), ("u32", "fast"), ("u32", "generic"), ("i8", "generic"), ("i16", "generic"),
         ("u8", "generic"), ("u16", "generic"), ("i64", "wide"), ("u64", "wide")]
CELL_IDS = [f"{t}-{e}" for t, e in CELLS]


@pytest.fixture(scope="module")
def ctx():
    c = chq.Context(0)
    c.set_option("split_rows", 1)
    c.set_option("enable_minus", 1)
    yield c
    c.close()


def ints(values, typ):
    return np.array(values, dtype=R.TYPES[typ].dtype)


def layouts(n):
    """index arrays: FULL rows repeating the table for the complete tiles, then one chunk for the incomplete tile; over all
    of them every table row occurs in both parts"""
    for s in range(0, n, CHUNK):
        yield np.concatenate([np.arange(FULL) % n, np.arange(s, min(s + CHUNK, n))])


def tile_kinds(cols):
    """a program over a 64-bit column is WIDE: pick_tile_kind gives it kind 2 whatever the option says"""
    return (2,) if any(v.dtype.itemsize == 8 for v in cols.values()) else TILE_KINDS


def batches(ctx, cols, null_col=None, table_mask=None):
    """(host batch, device batch, index array, null mask) per layout.  `null_col` gets the nulls: on NULL_ROWS, or where
    `table_mask` (in table order) says"""
    n = len(next(iter(cols.values())))
    for idx in layouts(n):
        mask = None
        if null_col is not None:
            if table_mask is not None:
                mask = table_mask[idx]
            else:
                mask = np.zeros(len(idx), dtype=bool)
                mask[list(NULL_ROWS)] = True
        rec = pa.RecordBatch.from_arrays([pa.array(v[idx], mask=mask if k == null_col else None) for k, v in cols.items()], names=list(cols))
        yield rec, chq.DeviceRecordBatch.from_host(rec, ctx), idx, mask


def first_diff(got, exp, cols, idx):
    if got.type != exp.type or len(got) != len(exp):
        return f"type {got.type} / {exp.type}, length {len(got)} / {len(exp)}"
    g, w = got.to_pylist(), exp.to_pylist()
    bad = [i for i in range(len(g)) if g[i] != w[i]]
    return f"{len(bad)} rows differ; " + "; ".join(f"row {i} { {k: int(c[idx[i]]) for k, c in cols.items()} } got {g[i]} want {w[i]}" for i in bad[:3])


def check_values(ctx, cols, forms, null_col=None, table_mask=None):
    """forms: [(sql, expected values as a numpy array in table order)].  The null mask applies to a form's result when the
    form reads the nullable column"""
    al = [[] for _ in cols]
    parsed = [(sql, parse_expr(sql), want) for sql, want in forms]
    for _, dev, idx, mask in batches(ctx, cols, null_col, table_mask):
        for sql, e, want in parsed:
            exp = pa.array(want[idx], mask=mask if null_col is not None and re.search(rf"\b{null_col}\b", sql) else None)
            for tk in tile_kinds(cols):
                ctx.set_option("tile_kind", tk)
                got = chq.compute_value(dev, al, e, ctx=ctx)[0]
                assert arrays_identical(got, exp), f"{sql} (tile_kind {tk}): {first_diff(got, exp, cols, idx)}"


def check_filter(ctx, cols, forms, null_col=None):
    """forms: [(sql, boolean keep mask in table order)]"""
    al = [[] for _ in cols]
    parsed = [(sql, parse_expr(sql), keep) for sql, keep in forms]
    for rec, dev, idx, mask in batches(ctx, cols, null_col):
        for sql, e, keep in parsed:
            # (a null operand makes the predicate null: the row is dropped)
            k = keep[idx] & ~mask if mask is not None and re.search(rf"\b{null_col}\b", sql) else keep[idx]
            exp = rec.filter(pa.array(k))
            for tk in tile_kinds(cols):
                ctx.set_option("tile_kind", tk)
                got = chq.filter_record(dev, al, e, ctx=ctx).to_host()
                assert batches_identical(got, exp), f"{sql} (tile_kind {tk}): {explain_diff(got, exp)}"


def expect_error(call, status, row, what=""):
    """the call raises (and so leaves no output) with the reference's status and row"""
    with pytest.raises(chq.ChqError) as ei:
        call()
    m = re.search(r"row (\d+)", str(ei.value))
    assert ei.value.code == R.STATUS[status] and m and int(m.group(1)) == row, f"{what}: want status {R.STATUS[status]} at row {row}, got {ei.value}"


def ok_pair_cols(typ, op):
    pairs, res = R.pair_table(typ), R.pair_results(typ, op)
    ok = R.ok_rows(typ, op)
    return {"x": ints([pairs[i][0] for i in ok], typ), "y": ints([pairs[i][1] for i in ok], typ)}, ints([res[i] for i in ok], typ)


def null_col_of(evaluator):
    return "x" if evaluator == "generic" else None


# ---------------------------------------------------------------------------------------------- values: x OP y
@pytest.mark.parametrize("op", R.OPS)
@pytest.mark.parametrize("typ,evaluator", CELLS, ids=CELL_IDS)
def test_arithmetic_through_compute_value(ctx, typ, evaluator, op):
    """project_kernel: x OP y on the `ok` pairs of the pair table ("i32-fast" with `/` `%` is the generic interpreter at
    every kind); for the 32-bit fast cells also the reversed column operand `x OP (y * one)`, FU_RSUB_I / FU_RSUB_U"""
    cols, want = ok_pair_cols(typ, op)
    forms = [(f"x {op} y", want)]
    if evaluator == "fast":
        cols["one"] = np.ones(len(want), dtype=want.dtype)
        forms.append((f"x {op} (y * one)", want))
    check_values(ctx, cols, forms, null_col_of(evaluator))


@pytest.mark.parametrize("op", R.OPS)
@pytest.mark.parametrize("typ,evaluator", CELLS, ids=CELL_IDS)
def test_arithmetic_through_filter_record(ctx, typ, evaluator, op):
    """filter_fused_kernel: `x OP y = z` with z the reference keeps every row; `= w`, w off by one in every seventh row,
    drops exactly those"""
    cols, want = ok_pair_cols(typ, op)
    every7 = np.arange(len(want)) % 7 == 0
    cols["z"] = want
    cols["w"] = want ^ every7.astype(want.dtype)
    check_filter(ctx, cols, [(f"x {op} y = z", np.ones(len(want), dtype=bool)), (f"x {op} y = w", ~every7)], null_col_of(evaluator))


@pytest.mark.parametrize("op", R.OPS)
@pytest.mark.parametrize("typ", ["i32", "u32", "i64", "u64"])
def test_arithmetic_through_filter_project(ctx, typ, op):
    """filter_project_kernel (`fuse` = 2, one launch): select x OP y as r from t where id >= 0 on non-null columns -- Int32 /
    UInt32 at kinds 0 and 1 (FASTK, `/` `%` generic), Int64 / UInt64 at kind 2"""
    cols, want = ok_pair_cols(typ, op)
    cols["id"] = np.arange(len(want), dtype=np.int32)
    sel = parse_select(f"select x {op} y as r from t where id >= 0")
    ctx.set_option("fuse", 2)
    try:
        for _, dev, idx, _ in batches(ctx, cols):
            exp = pa.RecordBatch.from_arrays([pa.array(want[idx])], names=["r"])
            for tk in (0, 1) if R.TYPES[typ].width == 32 else (2,):
                ctx.set_option("tile_kind", tk)
                got = chq.filter_project_record(sel.selection, sel.projection, dev, [[], [], []], ctx=ctx).to_host()
                assert ctx.last_stats()["launches"] == 1, "the two-step path ran instead of the fused kernel"
                assert batches_identical(got, exp, check_nullable=False), f"{op} (tile_kind {tk}): {explain_diff(got, exp)}"
    finally:
        ctx.set_option("fuse", 1)


@pytest.mark.parametrize("typ,op", TYPE_OPS, ids=TYPE_OP_IDS)
def test_null_slots_hide_errors(ctx, typ, op):
    """the whole pair table, failing pairs included, x null exactly on the failing rows: no error, `ok` rows exact, the rest
    null -- every failing pair of the table is on the device at once (generic interpreter / wide; y nullable instead of x
    gives the operand's validity the same job)"""
    pairs, res = R.pair_table(typ), R.pair_results(typ, op)
    fails = np.array([R.tag(r) != "ok" for r in res])
    assert fails.any() and not fails.all()
    want = ints([0 if f else r for f, r in zip(fails, res)], typ)
    for null_col in ("x", "y"):
        cols = {"x": ints([a for a, _ in pairs], typ), "y": ints([b for _, b in pairs], typ)}
        al, e = [[], []], parse_expr(f"x {op} y")
        for _, dev, idx, mask in batches(ctx, cols, null_col, fails):
            exp = pa.array(want[idx], mask=mask)
            for tk in tile_kinds(cols):
                ctx.set_option("tile_kind", tk)
                got = chq.compute_value(dev, al, e, ctx=ctx)[0]
                assert arrays_identical(got, exp), f"null {null_col} (tile_kind {tk}): {first_diff(got, exp, cols, idx)}"


# ---------------------------------------------------------------------------------------------- literal operands
def literal_forms(op):
    """(sql, f): f(x) is the reference of the form at Int32 x"""
    out = []
    for c in R.LITERAL_CONSTANTS + ((8,) if op in "/%" else ()):
        out += [(f"x {op} {c}", lambda x, c=c: R.arith(op, x, c, "i32")), (f"{c} {op} x", lambda x, c=c: R.arith(op, c, x, "i32")),
                (f"x {op} (0 - {c})", lambda x, c=c: R.arith(op, x, -c, "i32")), (f"(0 - {c}) {op} x", lambda x, c=c: R.arith(op, -c, x, "i32")),
                (f"{c} {op} (x + 0)", lambda x, c=c: R.arith(op, c, x, "i32")), (f"(0 - {c}) {op} (x + 0)", lambda x, c=c: R.arith(op, -c, x, "i32"))]
    return out


@pytest.mark.parametrize("op", R.OPS)
@pytest.mark.parametrize("evaluator", ["fast", "generic"])
def test_literal_operands_in_both_orders(ctx, evaluator, op):
    """Int32 x over the specials, each form on the rows where it is `ok`.  `x OP c`: a literal operand (for `/` `%` by 2^k
    the shortcut; by 3, 7, 46341, 2147483647 and by every negative constant the real division).  `c OP x`: LOAD const, column
    operand -- `8 / x`, `8 % x` are real divisions.  `c OP (x + 0)`: the reversed literal (FU_RSUB_I; IF_REV keeps `8 / ..`
    off the shortcut)"""
    sp = R.specials("i32")
    groups = {}
    for sql, f in literal_forms(op):
        res = [f(x) for x in sp]
        ok = tuple(i for i, r in enumerate(res) if R.tag(r) == "ok")
        assert ok, sql
        groups.setdefault(ok, []).append((sql, ints([res[i] for i in ok], "i32")))
    assert op not in "/%" or any(s == f"8 {op} x" for g in groups.values() for s, _ in g)
    for ok, forms in groups.items():
        check_values(ctx, {"x": ints([sp[i] for i in ok], "i32")}, forms, null_col_of(evaluator))


POW2_CELLS = [("i32", None), ("i32", "x"), ("i8", None), ("i16", None)]


@pytest.mark.parametrize("typ,null_col", POW2_CELLS, ids=["i32-fast", "i32-generic", "i8", "i16"])
def test_power_of_two_shortcut(ctx, typ, null_col):
    """x / 2^k and x % 2^k, k = 0..30, and the neighbour literals that must divide for real: FU_DIVP2_I / FU_REMP2_I on a
    non-null Int32 column, Interp::arith's own shortcut on a nullable one and on Int8 / Int16 columns (coerced to Int32).
    -1 / 2 = 0, INT32_MIN / 2^30 = -2, (INT32_MIN + 1) % 2^30 = -(2^30 - 1) are rows of the table"""
    xs, lits = R.pow2_table(typ)
    forms = []
    for c in lits:
        forms += [(f"x / {c}", ints([R.arith("/", x, c, "i32") for x in xs], "i32")), (f"x % {c}", ints([R.arith("%", x, c, "i32") for x in xs], "i32"))]
    check_values(ctx, {"x": ints(xs, typ)}, forms, null_col)


# ---------------------------------------------------------------------------------------------- widening
@pytest.mark.parametrize("l,r", R.MIXED_PAIRS, ids=[f"{l}+{r}" for l, r in R.MIXED_PAIRS])
def test_widening_through_mixed_arithmetic(ctx, l, r):
    """Interp::convert: both operand orders of `+` and `*` on the rows that are `ok` in the common type, and `<` on every
    row; the unsigned values with the high bit set must come out positive"""
    ct = R.common_type(l, r)
    pairs = [(a, b) for a in R.specials(l) for b in R.specials(r)]
    assert any(a > R.TYPES[l].hi // 2 for a, _ in pairs) or R.TYPES[l].signed
    for op in "+*":
        ok = [(a, b) for a, b in pairs if R.tag(R.arith(op, a, b, ct)) == "ok"]
        want = ints([R.arith(op, a, b, ct) for a, b in ok], ct)
        check_values(ctx, {"x": ints([a for a, _ in ok], l), "y": ints([b for _, b in ok], r)}, [(f"x {op} y", want), (f"y {op} x", want)])
    lt = np.array([a < b for a, b in pairs])
    gt = np.array([a > b for a, b in pairs])
    check_values(ctx, {"x": ints([a for a, _ in pairs], l), "y": ints([b for _, b in pairs], r)}, [("x < y", lt), ("y < x", gt), ("x >= y", ~lt)])


# ---------------------------------------------------------------------------------------------- comparisons
@pytest.mark.parametrize("typ,evaluator", CELLS, ids=CELL_IDS)
def test_comparisons_column_against_column(ctx, typ, evaluator):
    """all six operators on the whole pair table (no pair fails): FU_EQ / FU_LT_* / FU_GT_* with FU_NEGATE, Interp::compare"""
    pairs = R.pair_table(typ)
    cols = {"x": ints([a for a, _ in pairs], typ), "y": ints([b for _, b in pairs], typ)}
    forms = [(f"x {op} y", np.array([R.compare(op, a, b) for a, b in pairs])) for op in R.CMPS]
    check_values(ctx, cols, forms, null_col_of(evaluator))
    check_filter(ctx, cols, [forms[2], forms[5]], null_col_of(evaluator))


@pytest.mark.parametrize("nulls", [False, True], ids=["fast", "generic"])
def test_comparisons_against_literals(ctx, nulls):
    """Int32 column against 0, 1, 2147483646, 2147483647, -1, -2147483647, on either side.  Alone through filter_record:
    run_cmp_const in complete waves and run_fast in incomplete ones, with or without nulls.  Under AND a non-null column
    takes run_fast (FU_LT_I ..), a nullable one Interp::compare's literal branch; compute_value: project_kernel"""
    sp = R.specials("i32")
    x = ints(sp, "i32")
    cols = {"x": x, "id": np.arange(len(sp), dtype=np.int32)}
    forms = []
    for sql, c in R.CMP_LITERALS:
        assert c in sp
        for op in R.CMPS:
            forms += [(f"x {op} {sql}", np.array([R.compare(op, v, c) for v in sp])), (f"{sql} {op} x", np.array([R.compare(op, c, v) for v in sp]))]
            if op in ("<", ">=", "="):
                forms += [(f"x {op} {sql} and id >= 0", forms[-2][1]), (f"id >= 0 and {sql} {op} x", forms[-1][1])]
    check_filter(ctx, cols, forms, "x" if nulls else None)
    check_values(ctx, cols, [f for f in forms if " and " not in f[0]], "x" if nulls else None)


@pytest.mark.parametrize("typ", ["i64", "u64"])
def test_comparisons_of_64_bit_values_word_by_word(ctx, typ):
    """pairs that differ only in the high word or only in the low word, with either word's top bit set"""
    v = R.word_values(typ)
    pairs = [(a, b) for a in v for b in v]
    cols = {"x": ints([a for a, _ in pairs], typ), "y": ints([b for _, b in pairs], typ)}
    check_values(ctx, cols, [(f"x {op} y", np.array([R.compare(op, a, b) for a, b in pairs])) for op in R.CMPS])


@pytest.mark.parametrize("typ,evaluator", CELLS, ids=CELL_IDS)
def test_integer_to_boolean_under_and(ctx, typ, evaluator):
    """value != 0; the 64-bit values 2^32 and -2^32 (a zero low word) are true"""
    pairs = R.pair_table(typ)
    if R.TYPES[typ].width == 64:
        assert (2**32, 2**32) in pairs and R.to_bool(2**32) and (typ == "u64" or ((-2**32, 1) in pairs and R.to_bool(-2**32)))
    cols = {"x": ints([a for a, _ in pairs], typ), "y": ints([b for _, b in pairs], typ)}
    both = np.array([R.to_bool(a) and R.to_bool(b) for a, b in pairs])
    either = np.array([R.to_bool(a) or R.to_bool(b) for a, b in pairs])
    check_values(ctx, cols, [("x and y", both), ("y and x", both), ("x or y", either)], null_col_of(evaluator))


# ---------------------------------------------------------------------------------------------- errors
@pytest.mark.parametrize("typ,op", TYPE_OPS, ids=TYPE_OP_IDS)
def test_every_failing_pair_is_detected(ctx, typ, op):
    """every failing pair of the pair table is the first error of one short launch (one incomplete tile of at most 1 500
    rows): `ok` rows, the pair under test at a row that varies, then every other failing pair -- a missed detection shows
    up as a later row.  Tile kinds 0 / 1 / 2 rotate over the pairs; Int32 / UInt32 `+ - *` alternate a non-null column
    (FASTK) and a nullable one (generic, row 0 null)"""
    pairs, res = R.pair_table(typ), R.pair_results(typ, op)
    xa, ya = ints([a for a, _ in pairs], typ), ints([b for _, b in pairs], typ)
    ok, fails = np.array(R.ok_rows(typ, op)), np.array(R.failing_rows(typ, op))
    room = CHUNK - len(fails)
    assert room >= 100
    alternate = R.TYPES[typ].width == 32 and op in "+-*"
    al, e = [[], []], parse_expr(f"x {op} y")
    for i, f in enumerate(fails):
        p = 1 + (i * 37) % (room - 1)
        idx = np.concatenate([ok[(np.arange(p) + i) % len(ok)], fails[i:], fails[:i]])
        mask = None
        if alternate and (i // 3) % 2:
            mask = np.zeros(len(idx), dtype=bool)
            mask[0] = True
        rec = pa.RecordBatch.from_arrays([pa.array(xa[idx], mask=mask), pa.array(ya[idx])], names=["x", "y"])
        dev = chq.DeviceRecordBatch.from_host(rec, ctx)
        ctx.set_option("tile_kind", i % 3)
        expect_error(lambda: chq.compute_value(dev, al, e, ctx=ctx), res[f], p, f"{pairs[f]} (tile_kind {i % 3}, nullable {mask is not None})")


# one failing pair per failure class, per cell of the matrix
ROW_CELLS = [("i32", False), ("i32", True), ("u32", False), ("i8", False), ("i64", False)]
ENTRIES = ("compute_value", "filter_record", "filter_project_record")
N_ROWS = FULL + 1447      # not a multiple of 64


def class_pairs(typ):
    """[(op, class, (a, b), status)]: the first pair of every failure class of every operator"""
    out = []
    for op in R.OPS:
        for c, rows in sorted(R.class_members(typ, op).items()):
            if c != "other":
                out.append((op, c, R.pair_table(typ)[rows[0]], R.pair_results(typ, op)[rows[0]]))
    return out


def positions(tk):
    """rows of the FULL + PARTIAL layout where the row arithmetic can go wrong"""
    w, t = WAVE_ROWS[tk], TILE_ROWS[tk]
    return sorted({0, 63, 64, 65, w - 1, w, t, FULL - 1, FULL, N_ROWS - 1})


def run_entry(ctx, entry, dev, op):
    """x OP y over the batch through one of the three entry points"""
    if entry == "compute_value":
        return chq.compute_value(dev, [[], [], []], parse_expr(f"x {op} y"), ctx=ctx)
    if entry == "filter_record":
        return chq.filter_record(dev, [[], [], []], parse_expr(f"x {op} y = x"), ctx=ctx)
    sel = parse_select(f"select x {op} y as r from t where id >= 0")
    return chq.filter_project_record(sel.selection, sel.projection, dev, [[], [], []], ctx=ctx)


def error_batch(ctx, typ, failing, nullable=False):
    """N_ROWS rows of 1 OP 1 (`ok` for every operator and type) with the pairs of `failing` = {row: (a, b)} put in"""
    x, y = np.ones(N_ROWS, dtype=R.TYPES[typ].dtype), np.ones(N_ROWS, dtype=R.TYPES[typ].dtype)
    for row, (a, b) in failing.items():
        x[row], y[row] = ints([a], typ)[0], ints([b], typ)[0]
    mask = None
    if nullable:
        mask = np.zeros(N_ROWS, dtype=bool)
        mask[[r for r in (7, FULL + 3) if r not in failing]] = True
    rec = pa.RecordBatch.from_arrays([pa.array(x, mask=mask), pa.array(y), pa.array(np.arange(N_ROWS, dtype=np.int32))], names=["x", "y", "id"])
    return chq.DeviceRecordBatch.from_host(rec, ctx)


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("typ,nullable", ROW_CELLS, ids=["i32-fast", "i32-generic", "u32-fast", "i8-generic", "i64-wide"])
def test_reported_row_at_wave_tile_and_launch_boundaries(ctx, typ, nullable, entry):
    """one failing pair per failure class, alone in a batch of `ok` rows, at rows 0, 63, 64, 65, the last row of the first
    wave's span, the first row of the next wave and of the next workgroup, the last row of the last complete tile, the
    first row of the PARTIAL tile and the last row of the batch: status and row, at every tile kind, through compute_value,
    filter_record and filter_project_record (`fuse` = 2; a nullable column takes its two-step path)"""
    kinds = (2,) if R.TYPES[typ].width == 64 else TILE_KINDS
    rows = sorted({r for tk in kinds for r in positions(tk)})
    ctx.set_option("fuse", 2)
    try:
        for op, c, pair, status in class_pairs(typ):
            for row in rows:
                dev = error_batch(ctx, typ, {row: pair}, nullable)
                for tk in kinds:
                    ctx.set_option("tile_kind", tk)
                    expect_error(lambda: run_entry(ctx, entry, dev, op), status, row, f"{entry} {pair[0]} {op} {pair[1]} [{c}] (tile_kind {tk})")
    finally:
        ctx.set_option("fuse", 1)


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("typ,nullable", ROW_CELLS, ids=["i32-fast", "i32-generic", "u32-fast", "i8-generic", "i64-wide"])
def test_smallest_failing_row_wins_across_tiles_and_launches(ctx, typ, nullable, entry):
    """two and three failing rows at once, in different waves, tiles and launches (FULL and PARTIAL): the smallest row is
    reported -- with its own status where the rows fail differently -- whichever tile finishes first"""
    T = R.TYPES[typ]
    over = {"+": (T.hi, 1), "-": (T.lo, 1), "*": (T.hi, 2)}
    row_sets = [(FULL + 5, 300), (300, FULL + 5), (FULL + 700, 9000, 2500), (2500, FULL - 1, N_ROWS - 1), (FULL, FULL - 1), (N_ROWS - 1, FULL + 64),
                (2047, 2048), (15 * 1024 + 1023, 1023, 1024)]
    kinds = (2,) if T.width == 64 else TILE_KINDS
    ctx.set_option("fuse", 2)
    try:
        for op in R.OPS:
            # the first pair listed sits at the first row listed ... : a different status per row where the operator has two
            pairs = [over[op]] * 3 if op in over else ([(7, 0), (T.lo, -1), (0, 0)] if T.signed else [(7, 0), (T.hi, 0), (0, 0)])
            for rows in row_sets:
                failing = dict(zip(rows, pairs))
                first = min(rows)
                status = R.arith(op, *failing[first], typ)
                assert R.tag(status) != "ok" and all(R.tag(R.arith(op, *p, typ)) != "ok" for p in failing.values())
                dev = error_batch(ctx, typ, failing, nullable)
                for tk in kinds:
                    ctx.set_option("tile_kind", tk)
                    expect_error(lambda: run_entry(ctx, entry, dev, op), status, first, f"{entry} {op} rows {rows} (tile_kind {tk})")
    finally:
        ctx.set_option("fuse", 1)


@pytest.mark.parametrize("typ", ["i32", "u32", "i64"])
def test_projection_errors_follow_the_predicate(ctx, typ):
    """filter_project_record: a failing pair of the projection on a row the predicate drops raises nothing -- the fused
    kernel narrows the active rows to the survivors -- and the same pair on a kept row is reported.  (The rows ahead of it
    are all kept: when the fused kernel flags an error the call runs filter_record, then project_record on the survivors,
    and the row it reports counts project_record's input)"""
    T = R.TYPES[typ]
    kinds = (0, 1) if T.width == 32 else (2,)
    ctx.set_option("fuse", 2)
    try:
        for op, pair in (("+", (T.hi, 1)), ("*", (T.hi, 2)), ("/", (7, 0)), ("%", (7, 0))):
            for row in (65, 2048, FULL - 1, FULL, N_ROWS - 1):
                dev = error_batch(ctx, typ, {row: pair})
                drop = parse_select(f"select x {op} y as r from t where id <> {row}")
                behind = parse_select(f"select x {op} y as r from t where " + (f"id <> {N_ROWS - 2}" if row < N_ROWS - 2 else "id >= 0"))
                exp = pa.RecordBatch.from_arrays([pa.array(ints([R.arith(op, 1, 1, typ)] * (N_ROWS - 1), typ))], names=["r"])
                for tk in kinds:
                    ctx.set_option("tile_kind", tk)
                    got = chq.filter_project_record(drop.selection, drop.projection, dev, [[], [], []], ctx=ctx).to_host()
                    assert ctx.last_stats()["launches"] == 1, "the two-step path ran instead of the fused kernel"
                    assert batches_identical(got, exp, check_nullable=False), f"{op} row {row} (tile_kind {tk}): {explain_diff(got, exp)}"
                    expect_error(lambda: chq.filter_project_record(behind.selection, behind.projection, dev, [[], [], []], ctx=ctx),
                                 R.arith(op, *pair, typ), row, f"{op} row {row} (tile_kind {tk})")
    finally:
        ctx.set_option("fuse", 1)


@pytest.mark.parametrize("typ", ["i32", "i64", "i8"])
def test_node_order_beats_row_order(ctx, typ):
    """the first failing node in the reference's evaluation order decides, then its smallest row: `(x + y) / z` with a zero
    divisor early and an overflowing sum late reports the overflow; `(p / z) + (x * y)` (a numeric temporary: kind 2) with an
    overflowing product early and a zero divisor late reports the divide by zero.  The oracle agrees on the status"""
    T = R.TYPES[typ]
    early, late = 10, FULL + 1000
    one = np.ones(N_ROWS, dtype=T.dtype)
    cases = []
    x, z = one.copy(), one.copy()
    x[late], z[early] = T.hi, 0
    cases.append(("(x + y) / z", {"x": x, "y": one, "z": z, "p": one}))
    x, y, z = one.copy(), one.copy(), one.copy()
    x[early], y[early], z[late] = T.hi, 2, 0
    cases.append(("(p / z) + (x * y)", {"x": x, "y": y, "z": z, "p": one}))
    for k, (sql, cols) in enumerate(cases):
        x, y, z, p = ([int(v) for v in cols[n]] for n in "xyzp")
        if k == 0:
            s = [R.arith("+", a, b, typ) for a, b in zip(x, y)]
            nodes = [s, [R.arith("/", a, b, typ) if R.tag(a) == "ok" else None for a, b in zip(s, z)]]
            want = (R.OVERFLOW, late)
        else:
            nodes = [[R.arith("/", a, b, typ) for a, b in zip(p, z)], [R.arith("*", a, b, typ) for a, b in zip(x, y)]]
            want = (R.DIV_ZERO, late)
        assert R.first_error(nodes) == want and sum(R.tag(r) != "ok" for n in nodes for r in n if r is not None) == 2
        rec = pa.RecordBatch.from_arrays([pa.array(v) for v in cols.values()], names=list(cols))
        with pytest.raises(O.OracleError) as oe:
            O.compute_value(rec, [[]] * 4, parse_expr(sql))
        assert oe.value.code == R.STATUS[want[0]]
        dev = chq.DeviceRecordBatch.from_host(rec, ctx)
        for tk in (2,) if T.width == 64 else TILE_KINDS:
            ctx.set_option("tile_kind", tk)
            expect_error(lambda: chq.compute_value(dev, [[]] * 4, parse_expr(sql), ctx=ctx), *want, f"{sql} (tile_kind {tk})")
            expect_error(lambda: chq.filter_record(dev, [[]] * 4, parse_expr(f"{sql} = x"), ctx=ctx), *want, f"{sql} = x (tile_kind {tk})")
