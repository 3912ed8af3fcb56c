"""GPU: float arithmetic, comparisons, conversions and literals on IEEE edge values, bit for bit (NaN payloads included)
against the exact reference of tests/float_reference.py -- the tables tests/test_float_reference.py ties to numpy and the
oracle on the CPU tier.

Where every row runs.  The context forces the large-batch launch structure (`split_rows` = 1: complete tiles in the
FULL-only instantiation, the incomplete last tile in a PARTIAL launch).  A batch is 16 384 rows of a table -- one complete
tile of `tile_kind` 0, eight of kinds 1 and 2 -- followed by one chunk of at most 1 500 rows, the incomplete tile.  A table
of up to 16 384 rows is repeated to fill the complete part; the 65 536-row Float16 sweep takes its four quarters in turn.
The chunks walk the whole table, so every row is evaluated in a complete tile of the FULL launch and in the incomplete tile
of the PARTIAL launch.

Which instantiation runs (filter.cpp: encode_fast_uops, pick_tile_kind; kernels.hip: launch_filter / launch_project /
launch_filter_project) is decided by construction -- `last_stats` does not report it:
  * tile kinds 0 and 1, FASTK (run_fast): programs over non-null Int32 / UInt32 / Float32 columns and 32-bit literals,
    EXCEPT Float32 `%` (fmod is never pre-decoded).  run_fast also evaluates the incomplete waves of the PARTIAL tile
    (range-checked loads).  A lone `column <cmp> literal` -- with or without nulls in the column -- takes run_cmp_const in
    complete waves and run_fast in incomplete ones.
  * tile kinds 0 and 1, generic interpreter (Interp::arith / compare / convert, WIDE = false): the same programs when a
    column has a validity bitmap (a few nulls sit on rows of the complete part whose values occur elsewhere without one;
    a lone `column <cmp> literal` is the exception above), and Float32 `%` always.
  * tile kind 2 (WIDE = true, generic interpreter only): every program that touches a 64-bit or Float16 value, whatever the
    `tile_kind` option says -- those run ONE pass here -- and 32-bit programs when the option forces kind 2.  Float32
    arithmetic next to 64-bit values is written `(x OP y) * one64`.
  * filter_project_kernel (`fuse` = 2) is one launch with no FULL / PARTIAL split: kinds 0 and 1 for 32-bit programs (FASTK
    for + - * /, generic for `%`), kind 2 for Float64.
The tests below name the cells of this matrix they cover: "f32-fast" = FASTK at kinds 0 / 1 plus the kind-2 interpreter on
non-null columns; "f32-generic" = the interpreter at kinds 0 / 1 / 2 on a nullable column; "wide" = kind 2 alone.
"""
import functools
import re

import numpy as np
import pyarrow as pa
import pytest

import chapterhouseqe_amd as chq
from chapterhouseqe_amd.sqlparse import parse_expr, parse_select

from . import float_reference as R
from .helpers import arrays_identical, batches_identical, explain_diff

pytestmark = pytest.mark.gpu

FULL, CHUNK = 16384, 1500
TILE_KINDS = (0, 1, 2)
NULL_ROWS = (5, 4096 + 77, 2 * 4096 + 1031, 3 * 4096 + 4000)
PA = {"f16": pa.float16(), "f32": pa.float32(), "f64": pa.float64()}
ONE = {f: R.encode(0, 1, f) for f in R.FORMATS}


@pytest.fixture(scope="module")
def ctx():
    c = chq.Context(0)
    c.set_option("split_rows", 1)
    c.set_option("enable_minus", 1)
    yield c
    c.close()


def layouts(n):
    """index arrays: FULL rows for the complete tiles, then one chunk for the incomplete tile; over all of them every table
    row occurs in both parts (a table longer than FULL supplies its FULL-row blocks in turn)"""
    blocks = -(-n // FULL)
    starts = list(range(0, n, CHUNK))
    assert len(starts) >= blocks
    for i, s in enumerate(starts):
        base = (np.arange(FULL) + FULL * (i % blocks)) % n
        yield np.concatenate([base, np.arange(s, min(s + CHUNK, n))])


def tile_kinds(cols):
    """a program over a 64-bit or Float16 column is WIDE: pick_tile_kind gives it kind 2 whatever the option says"""
    wide = any(v.dtype.itemsize == 8 or v.dtype == np.float16 for v in cols.values())
    return (2,) if wide else TILE_KINDS


def fl(bits, fmt):
    return np.asarray(bits, dtype=R.FORMATS[fmt].utype).view(R.FORMATS[fmt].dtype)


def column(values, idx, mask=None):
    v = values[idx]
    typ = pa.float16() if v.dtype == np.float16 else None
    return pa.array(v, typ, mask=mask)


def batches(ctx, cols, null_col=None):
    """(device batch, index array, null mask) per layout; `null_col` gets the nulls"""
    n = len(next(iter(cols.values())))
    for idx in layouts(n):
        mask = None
        if null_col is not None:
            mask = np.zeros(len(idx), dtype=bool)
            mask[[r for r in NULL_ROWS if r < len(idx)]] = True
        rec = pa.RecordBatch.from_arrays([column(v, idx, mask if k == null_col else None) for k, v in cols.items()], names=list(cols))
        yield rec, chq.DeviceRecordBatch.from_host(rec, ctx), idx, mask


def check_values(ctx, cols, forms, null_col=None):
    """forms: [(sql, expected values as a numpy array in table order)]"""
    al = [[] for _ in cols]
    parsed = [(sql, parse_expr(sql), want) for sql, want in forms]
    for _, dev, idx, mask in batches(ctx, cols, null_col):
        for sql, e, want in parsed:
            exp = column(want, idx, mask)
            for tk in tile_kinds(cols):
                ctx.set_option("tile_kind", tk)
                got = chq.compute_value(dev, al, e, ctx=ctx)[0]
                assert arrays_identical(got, exp, nan_payload=True), f"{sql} (tile_kind {tk}): {first_diff(got, exp, cols, idx)}"


def check_filter(ctx, cols, forms, null_col=None):
    """forms: [(sql, boolean keep mask in table order)]"""
    al = [[] for _ in cols]
    parsed = [(sql, parse_expr(sql), keep) for sql, keep in forms]
    for rec, dev, idx, mask in batches(ctx, cols, null_col):
        for sql, e, keep in parsed:
            # (a null operand makes the predicate null: the row is dropped -- only where the predicate reads that column)
            k = keep[idx] & ~mask if mask is not None and re.search(rf"\b{null_col}\b", sql) else keep[idx]
            exp = rec.filter(pa.array(k))
            for tk in tile_kinds(cols):
                ctx.set_option("tile_kind", tk)
                got = chq.filter_record(dev, al, e, ctx=ctx).to_host()
                assert batches_identical(got, exp, nan_payload=True), f"{sql} (tile_kind {tk}): {explain_diff(got, exp)}"


def first_diff(got, exp, cols, idx):
    g, w = got.to_pylist(), exp.to_pylist()
    raw = lambda a: a.fill_null(0).to_numpy(zero_copy_only=False).view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[max(1, a.type.bit_width // 8)]) if not pa.types.is_boolean(a.type) else np.asarray(a.fill_null(False))
    if got.type != exp.type or len(g) != len(w):
        return f"type {got.type} / {exp.type}, length {len(g)} / {len(w)}"
    rg, rw = raw(got), raw(exp)
    bad = [i for i in range(len(g)) if (g[i] is None) != (w[i] is None) or (w[i] is not None and rg[i] != rw[i])]
    show = lambda v: {k: hex(int(c[v].view({2: np.uint16, 4: np.uint32, 8: np.uint64}[c.dtype.itemsize]))) if c.dtype.kind == "f" else int(c[v]) for k, c in cols.items()}
    return f"{len(bad)} rows differ; " + "; ".join(f"row {i} {show(idx[i])} got {rg[i]:#x} want {rw[i]:#x}" for i in bad[:3])


# ---------------------------------------------------------------------------------------------- reference pieces
def lit_bits(text):
    return R.parse_literal(text)


@functools.lru_cache(maxsize=None)
def arith_const(op, fmt, side, lit):
    """reference of `x op <literal>` (side "r") or `<literal> op x` (side "l") over the pair table's left column (Float32 or
    Float64; a Float32 literal against a Float64 column is widened exactly)"""
    c = lit_bits(lit)
    if fmt == "f64":
        c = R.convert_float(c, "f32", "f64")
    vals = [int(x) for x in R.pair_table(fmt)[0]]
    return fl([R.arith(op, x, c, fmt) if side == "r" else R.arith(op, c, x, fmt) for x in vals], fmt)


def pair_cols(fmt):
    a, b = R.pair_table(fmt)
    return {"x": fl(a, fmt), "y": fl(b, fmt)}


ARITH_CASES = [("f32", "fast"), ("f32", "generic"), ("f32", "wide"), ("f64", "wide"), ("f16", "wide")]


@pytest.mark.parametrize("op", R.OPS)
@pytest.mark.parametrize("fmt,evaluator", ARITH_CASES, ids=[f"{f}-{e}" for f, e in ARITH_CASES])
def test_arithmetic_through_compute_value(ctx, fmt, evaluator, op):
    """project_kernel: x OP y on the pair table; for Float32 (fast and generic) and Float64 also x OP literal and literal OP x
    -- the IF_REV paths, FU_RSUB_F / FU_RDIV_F.  ("f32-fast" with `%` is the generic interpreter at every kind)"""
    cols = pair_cols(fmt)
    want = R.table_result("pairs", op, fmt)
    if evaluator == "wide" and fmt == "f32":
        cols["one64"] = np.ones(R.P)
        w64 = [R.arith("*", R.convert_float(int(r), "f32", "f64"), ONE["f64"], "f64") for r in want]
        forms = [(f"(x {op} y) * one64", fl(w64, "f64"))]
    else:
        forms = [(f"x {op} y", fl(want, fmt))]
    if fmt == "f32" and evaluator != "wide" or fmt == "f64":
        for lit in R.ARITH_LITERALS:
            forms += [(f"x {op} {lit}", arith_const(op, fmt, "r", lit)), (f"{lit} {op} x", arith_const(op, fmt, "l", lit))]
    check_values(ctx, cols, forms, null_col="x" if evaluator == "generic" else None)


@pytest.mark.parametrize("op", R.OPS)
def test_float16_arithmetic_on_every_pattern(ctx, op):
    """all 65 536 halves as the left operand: the two roundings, NaN payloads through the round-back (kind 2, 44 batches)"""
    a, b = R.f16_sweep()
    check_values(ctx, {"x": fl(a, "f16"), "y": fl(b, "f16")}, [(f"x {op} y", fl(R.table_result("sweep", op, "f16"), "f16"))])


@pytest.mark.parametrize("op", R.OPS)
@pytest.mark.parametrize("fmt", list(R.FORMATS))
def test_arithmetic_through_filter_record(ctx, fmt, op):
    """filter_fused_kernel: `x OP y = z` (float `=` is bitwise).  z = the reference's bits keeps every row; bit 0 flipped in
    every seventh row drops exactly those"""
    cols = pair_cols(fmt)
    want = R.table_result("pairs", op, fmt)
    every7 = np.arange(R.P) % 7 == 0
    cols["z"] = fl(want, fmt)
    cols["w"] = fl(want ^ every7.astype(want.dtype), fmt)
    check_filter(ctx, cols, [(f"x {op} y = z", np.ones(R.P, dtype=bool)), (f"x {op} y = w", ~every7)])


@pytest.mark.parametrize("op", R.OPS)
@pytest.mark.parametrize("fmt", ["f32", "f64"])
def test_arithmetic_through_filter_project(ctx, fmt, op):
    """filter_project_kernel (`fuse` = 2, one launch): select x OP y as r from t where id >= 0 on non-null columns --
    Float32 at kinds 0 and 1 (FASTK, `%` generic), Float64 at kind 2"""
    cols = pair_cols(fmt)
    cols["id"] = np.arange(R.P, dtype=np.int32)
    want = fl(R.table_result("pairs", op, fmt), fmt)
    sel = parse_select(f"select x {op} y as r from t where id >= 0")
    ctx.set_option("fuse", 2)
    try:
        for _, dev, idx, _ in batches(ctx, cols):
            exp = pa.RecordBatch.from_arrays([pa.array(want[idx])], names=["r"])
            for tk in (0, 1) if fmt == "f32" else (2,):
                ctx.set_option("tile_kind", tk)
                got = chq.filter_project_record(sel.selection, sel.projection, dev, [[], [], []], ctx=ctx).to_host()
                assert ctx.last_stats()["launches"] == 1, "the two-step path ran instead of the fused kernel"
                assert batches_identical(got, exp, check_nullable=False, nan_payload=True), f"{op} (tile_kind {tk}): {explain_diff(got, exp)}"
    finally:
        ctx.set_option("fuse", 1)


# ---------------------------------------------------------------------------------------------- comparisons
CMP_CASES = [("f32", None), ("f32", "x"), ("f64", None), ("f16", None)]


@pytest.mark.parametrize("fmt,null_col", CMP_CASES, ids=["f32-fast", "f32-generic", "f64-wide", "f16-wide"])
def test_comparisons_column_against_column(ctx, fmt, null_col):
    a, b = R.pair_table(fmt)
    forms = [(f"x {op} y", R.compare_bits(op, a, b, fmt)) for op in R.CMPS]
    check_values(ctx, pair_cols(fmt), forms, null_col)


def constants():
    """(sql, Float32 bits): the literal list and the three constants with the sign bit set"""
    return [(t, lit_bits(t)) for t in R.LITERALS] + [(f"({sql})", ref()) for sql, _, ref in R.SIGNED_CONSTANTS]


def against_constant(fmt, col_bits, c):
    """the column's and the constant's bits in the common type of the comparison"""
    if fmt == "f64":
        return "f64", [int(v) for v in col_bits], R.convert_float(c, "f32", "f64")
    if fmt == "f16":
        return "f32", [R.convert_float(int(v), "f16", "f32") for v in col_bits], c
    return "f32", [int(v) for v in col_bits], c


@pytest.mark.parametrize("k", range(len(R.LITERALS) + len(R.SIGNED_CONSTANTS)))
@pytest.mark.parametrize("fmt,null_col", CMP_CASES, ids=["f32-fast", "f32-generic", "f64-wide", "f16-wide"])
def test_comparisons_against_literals_through_filter_record(ctx, fmt, null_col, k):
    """each column against every literal, on either side.  Alone (`column <cmp> literal`), a Float32 column takes
    run_cmp_const -- for a literal with the sign bit set, its keyed arm -- nullable or not (kind 2: Interp::compare).  Under
    AND a non-null column takes run_fast (FU_LT_I / FU_LT_FKC), a nullable one Interp::compare with a literal operand"""
    a, b = R.pair_table(fmt)
    cols = pair_cols(fmt)
    cols["id"] = np.arange(R.P, dtype=np.int32)
    sql, c = constants()[k]
    forms = []
    for name, bits in (("x", a), ("y", b)):
        t, vals, cc = against_constant(fmt, bits, c)
        kv = np.array([R.total_order_key(v, t) for v in vals], dtype=np.int64)
        kc = R.total_order_key(cc, t)
        assert all((R.total_order_key(v, t) == kc) == (v == cc) for v in vals[:64])
        right = {"=": kv == kc, "<>": kv != kc, "<": kv < kc, "<=": kv <= kc, ">": kv > kc, ">=": kv >= kc}
        left = {"=": kv == kc, "<>": kv != kc, "<": kc < kv, "<=": kc <= kv, ">": kc > kv, ">=": kc >= kv}
        for op in R.CMPS:
            forms += [(f"{name} {op} {sql}", right[op]), (f"{sql} {op} {name}", left[op])]
            if name == "x" and op in ("<", ">="):
                forms += [(f"{name} {op} {sql} and id >= 0", right[op]), (f"id >= 0 and {sql} {op} {name}", left[op])]
    check_filter(ctx, cols, forms, null_col)


# ---------------------------------------------------------------------------------------------- conversions
@pytest.mark.parametrize("nulls", [False, True], ids=["fast", "generic"])
@pytest.mark.parametrize("typ", ["i32", "u32", "i8", "i16", "u8", "u16"])
def test_integer_to_float32_conversions(ctx, typ, nulls):
    """FO_COL_I2F / FO_COL_U2F / FU_CVT_* (fast: Int32 / UInt32 at kinds 0 and 1) and Interp::convert (nullable columns, the
    8- and 16-bit types, and kind 2)"""
    vals = R.int_table(typ)
    n = len(vals)
    xs = np.array([R.specials("f32")[(7 * i) % 52] for i in range(n)], dtype=np.uint32)
    conv = [R.convert_int(v, "f32") for v in vals]
    cols = {"i": np.array(vals, dtype=R.INT_TYPES[typ][0]), "x": fl(xs, "f32")}
    one = ONE["f32"]
    forms = [("i * 1.0", fl([R.arith("*", c, one, "f32") for c in conv], "f32")), ("1.0 * i", fl([R.arith("*", one, c, "f32") for c in conv], "f32")),
             ("x / i", fl([R.arith("/", int(x), c, "f32") for x, c in zip(xs, conv)], "f32")),
             ("i / x", fl([R.arith("/", c, int(x), "f32") for x, c in zip(xs, conv)], "f32"))]
    check_values(ctx, cols, forms, null_col="i" if nulls else None)


@pytest.mark.parametrize("typ", ["i64", "u64", "i32", "u32"])
def test_integer_to_float64_conversions(ctx, typ):
    vals = R.int_table(typ)
    cols = {"l": np.array(vals, dtype=R.INT_TYPES[typ][0]), "one64": np.ones(len(vals))}
    want = fl([R.arith("*", R.convert_int(v, "f64"), ONE["f64"], "f64") for v in vals], "f64")
    check_values(ctx, cols, [("l * one64", want), ("one64 * l", want)])


@pytest.mark.parametrize("src,dst", [("f32", "f64"), ("f16", "f32"), ("f16", "f64")])
def test_float_widening_through_mixed_arithmetic(ctx, src, dst):
    """a cast quiets a signalling NaN and keeps its payload; subnormals widen exactly"""
    a, _ = R.pair_table(src)
    cols = {"x": fl(a, src), "one": np.ones(R.P, dtype=R.FORMATS[dst].dtype)}
    want = fl([R.arith("*", R.convert_float(int(v), src, dst), ONE[dst], dst) for v in a], dst)
    check_values(ctx, cols, [("x * one", want), ("one * x", want)])


# ---------------------------------------------------------------------------------------------- to-Boolean, literals
@pytest.mark.parametrize("fmt,null_col", CMP_CASES, ids=["f32-fast", "f32-generic", "f64-wide", "f16-wide"])
def test_float_to_boolean_under_and(ctx, fmt, null_col):
    """a subnormal is true, -0.0 is false, a NaN is true"""
    sp = np.array(R.specials(fmt), dtype=R.FORMATS[fmt].utype)
    want = np.array([R.to_bool(int(v), fmt) for v in sp])
    F = R.FORMATS[fmt]
    assert want[list(sp).index(1)] and not want[list(sp).index(F.sign_bit)] and want[list(sp).index(F.inf_bits | F.quiet_bit)]
    check_values(ctx, {"x": fl(sp, fmt), "t": np.ones(len(sp), dtype=bool)}, [("x and t", want), ("t and x", want)], null_col)


@pytest.mark.parametrize("nulls", [False, True], ids=["fast", "generic"])
def test_literals_round_at_parse_time(ctx, nulls):
    """`x = <literal>` keeps exactly the rows whose bits equal parse_literal(text): alone (run_cmp_const, with nulls too) and
    under AND (run_fast; with nulls Interp::compare)"""
    a, _ = R.pair_table("f32")
    lits = [lit_bits(t) for t in R.LITERALS]
    near = [v for c in lits for v in (c, c ^ 1, c | 0x80000000)]
    x = np.concatenate([a[: R.P - len(near)], np.array(near, dtype=np.uint32)])
    cols = {"x": fl(x, "f32"), "id": np.arange(R.P, dtype=np.int32)}
    forms = [(f"x = {t}", x == c) for t, c in zip(R.LITERALS, lits)] + [(f"{t} = x", x == c) for t, c in zip(R.LITERALS, lits)]
    forms += [(f"x = {t} and id >= 0", x == c) for t, c in zip(R.LITERALS, lits)]
    assert all(k.any() for _, k in forms)
    check_filter(ctx, cols, forms, "x" if nulls else None)
