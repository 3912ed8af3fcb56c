"""CPU: CAST / TRY_CAST without a GPU.  The tests' reference (tests/cast_reference.py) against pyarrow and sqlite3 where they
agree with the library's rules; the grammar (CAST, TRY_CAST, `::`); the library's host half (typing, status codes, constant
folding with the per-row code the device runs) through `chq_plan_describe`; that per-row code alone in a stand-alone program
under the address and undefined-behaviour sanitizers; and the row counts tests/test_gpu_cast.py uses to reach the second
round of every capped grid, held to the sources."""
import os
import re
import shutil
import sqlite3
import subprocess

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest

import chapterhouseqe_amd as chq
from chapterhouseqe_amd import sqlast as A
from chapterhouseqe_amd.sqlparse import SqlParseError, parse_expr, parse_select

from . import cast_reference as R
from . import float_reference as F
from . import int_reference as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "chapterhouseqe_amd", "csrc")


def rows(src, dst, values=None):
    values = R.edges(src) if values is None else values
    return R.cast_rows(values, [True] * len(values), src, dst)


# ---- the reference against pyarrow and sqlite3, where they agree --------------------------------------------------------------
@pytest.mark.parametrize("src", R.INTS)
def test_reference_int_to_int_agrees_with_pyarrow_in_range(src):
    for dst in R.INTS:
        vals = [v for v in R.int_edges(src) if R.cast_value(v, src, dst) is not R.FAIL]
        assert len(vals) >= 5, (src, dst)
        got = pc.cast(pa.array(vals, R.ARROW[src]), R.ARROW[dst]).to_pylist()
        assert got == rows(src, dst, vals)[0], (src, dst)
        # and what the reference fails, pyarrow's safe cast refuses
        for v in [v for v in R.int_edges(src) if R.cast_value(v, src, dst) is R.FAIL][:6]:
            with pytest.raises(pa.ArrowInvalid):
                pc.cast(pa.array([v], R.ARROW[src]), R.ARROW[dst])


def test_reference_to_utf8_agrees_with_pyarrow():
    for src in R.INTS:
        vals = R.int_edges(src)
        assert pc.cast(pa.array(vals, R.ARROW[src]), pa.utf8()).to_pylist() == [b.decode() for b in rows(src, "utf8", vals)[0]], src
    assert pc.cast(pa.array([True, False]), pa.utf8()).to_pylist() == ["true", "false"] == [b.decode() for b in rows("bool", "utf8", [True, False])[0]]
    for src in R.INTS:   # 1 to 20 bytes
        lens = [len(b) for b in rows(src, "utf8")[0]]
        assert min(lens) == 1 and max(lens) <= 20
    assert max(len(b) for b in rows("i64", "utf8")[0]) == 20 == max(len(b) for b in rows("u64", "utf8")[0])


@pytest.mark.parametrize("dst", R.INTS)
def test_reference_utf8_to_int_agrees_with_pyarrow(dst):
    pinned = [s for s in R.string_edges() if re.fullmatch(rb"-?[0-9]+", s)]
    assert len(pinned) > 40
    for s in pinned:
        want = R.cast_value(s, "utf8", dst)
        try:
            got = pc.cast(pa.array([s.decode()]), R.ARROW[dst]).to_pylist()[0]
        except pa.ArrowInvalid:
            got = R.FAIL
        assert got == want, (s, dst)
    # the library's own answers where pyarrow differs: a leading `+` is accepted, a hexadecimal spelling is not
    assert R.cast_value(b"+1", "utf8", dst) == 1 and R.cast_value(b"+0", "utf8", dst) == 0 and R.cast_value(b"0x10", "utf8", dst) is R.FAIL
    assert R.cast_value(b"-0", "utf8", dst) == (0 if I.TYPES[dst].signed else R.FAIL)
    for s in (b"", b"+", b"-", b" 1", b"1 ", b"1.0", b"1e3", b"1\x002", "١٢٣".encode(), "１２".encode()):
        assert R.cast_value(s, "utf8", dst) is R.FAIL, s
    assert R.cast_value(b"0" * 25 + b"12", "utf8", dst) == 12


@pytest.mark.parametrize("src", ("f32", "f64"))
def test_reference_float_to_int_agrees_with_pyarrow_on_truncated_values(src):
    FM = F.FORMATS[src]
    for dst in R.INTS:
        ok = [b for b in R.float_edges(src) if R.cast_value(b, src, dst) is not R.FAIL]
        assert len(ok) > 20, (src, dst)
        arr = pa.array(np.array(ok, dtype=FM.utype).view(FM.dtype), R.ARROW[src])
        assert pc.cast(pc.trunc(arr), R.ARROW[dst]).to_pylist() == rows(src, dst, ok)[0], (src, dst)
    enc = lambda q: F.encode(q < 0, abs(q), src)
    from fractions import Fraction as Q
    assert R.cast_value(enc(Q(-9, 10)), src, "u8") == 0 and R.cast_value(enc(Q(-9, 10)), src, "i8") == 0 and R.cast_value(FM.sign_bit, src, "u64") == 0
    assert R.cast_value(enc(Q(-1)), src, "u8") is R.FAIL and R.cast_value(enc(Q(2**63)), src, "i64") is R.FAIL
    assert R.cast_value(enc(Q(2**63)), src, "u64") == 2**63 and R.cast_value(enc(Q(2**64)), src, "u64") is R.FAIL
    assert R.cast_value(enc(Q(-2**63)), src, "i64") == -2**63
    for b in (FM.inf_bits, FM.inf_bits | FM.sign_bit, FM.default_nan, FM.inf_bits | 1):
        assert R.cast_value(b, src, "i32") is R.FAIL


def test_reference_int_to_float_agrees_with_pyarrow_where_exact():
    for src in R.INTS:
        for dst, bound in (("f32", 1 << 24), ("f64", 1 << 53)):
            vals = [v for v in R.int_edges(src) if abs(v) <= bound]
            FM = F.FORMATS[dst]
            got = pc.cast(pa.array(vals, R.ARROW[src]), R.ARROW[dst]).to_numpy(zero_copy_only=False).view(FM.utype).tolist()
            assert got == rows(src, dst, vals)[0], (src, dst)
    # beyond: one rounding to nearest even, Float16 to infinity past 65504 + half an ulp
    assert R.cast_value((1 << 24) + 1, "i32", "f32") == F.encode(0, 1 << 24, "f32") and R.cast_value((1 << 24) + 3, "i32", "f32") == F.encode(0, (1 << 24) + 4, "f32")
    assert R.cast_value(65519, "i32", "f16") == 0x7BFF and R.cast_value(65520, "i32", "f16") == 0x7C00 and R.cast_value(-65520, "i32", "f16") == 0xFC00
    assert R.cast_value(2049, "i16", "f16") == F.encode(0, 2048, "f16") and R.cast_value(2051, "i16", "f16") == F.encode(0, 2052, "f16")
    # numpy rounds integers to float once too
    for src in ("i64", "u64"):
        vals = R.int_edges(src)
        for dst in ("f32", "f64"):
            FM = F.FORMATS[dst]
            assert np.array(vals, I.TYPES[src].dtype).astype(FM.dtype).view(FM.utype).tolist() == rows(src, dst, vals)[0], (src, dst)


def test_reference_float_to_float_agrees_with_pyarrow():
    bits = [b for b in R.float_edges("f64") if not F.is_nan(b, "f64")]
    arr = pa.array(np.array(bits, dtype=np.uint64).view(np.float64))
    got = pc.cast(arr, pa.float32(), safe=False).to_numpy(zero_copy_only=False).view(np.uint32).tolist()
    assert got == rows("f64", "f32", bits)[0]
    assert R.cast_value(F.encode(0, 2**128, "f64"), "f64", "f32") == F.FORMATS["f32"].inf_bits      # overflow to infinity
    wide = R.float_edges("f32")
    back = [b for b in wide if not F.is_nan(b, "f32")]
    arr32 = pa.array(np.array(back, dtype=np.uint32).view(np.float32))
    assert pc.cast(arr32, pa.float64()).to_numpy(zero_copy_only=False).view(np.uint64).tolist() == rows("f32", "f64", back)[0]
    # a NaN keeps its sign and the top of its payload, quiet
    assert R.cast_value(0xFFF0000000000001 | (0x15 << 40), "f64", "f32") == 0xFFC00000 | (0x15 << 11)
    assert R.cast_value(0x7F800001, "f32", "f64") == 0x7FF8000020000000 and R.cast_value(0xFE01, "f16", "f32") == 0xFFC00000 | (0x201 << 13)


def test_reference_booleans():
    for src in R.INTS:
        assert rows(src, "bool")[0] == [v != 0 for v in R.int_edges(src)]
    for src in R.FLOATS:
        FM = F.FORMATS[src]
        assert R.cast_value(FM.sign_bit, src, "bool") is False and R.cast_value(FM.default_nan, src, "bool") is True and R.cast_value(1, src, "bool") is True
    for dst in R.INTS:
        assert rows("bool", dst, [False, True])[0] == [0, 1]
    for dst in R.FLOATS:
        assert rows("bool", dst, [False, True])[0] == [0, F.encode(0, 1, dst)]
    ok = R.clean_rows("utf8", "bool")
    assert pc.cast(pa.array([s.decode() for s in ok if s.strip() == s and s.lower() in (b"true", b"false", b"1", b"0")]), pa.bool_()).to_pylist() == \
        [R.cast_value(s, "utf8", "bool") for s in ok if s.strip() == s and s.lower() in (b"true", b"false", b"1", b"0")]
    assert len(R.failing_rows("utf8", "bool")) >= 5 and len(ok) >= 10


def test_reference_agrees_with_sqlite_on_integral_text():
    db = sqlite3.connect(":memory:")
    for s in R.string_edges():
        if not re.fullmatch(rb"[+-]?[0-9]+", s):
            continue
        want = R.cast_value(s, "utf8", "i64")
        if want is R.FAIL:
            continue   # (sqlite saturates out-of-range text)
        assert db.execute("select cast(? as integer)", (s.decode(),)).fetchone()[0] == want, s
    for v in R.int_edges("i64"):
        assert db.execute("select cast(? as text)", (v,)).fetchone()[0].encode() == R.cast_value(v, "i64", "utf8"), v


def test_cast_rows_shape():
    vals, valid, failed = R.cast_rows([1, 300, 5, 400], [True, False, True, True], "i32", "i8")
    assert (vals, valid, failed) == ([1, 0, 5, 0], [True, False, True, False], 3)
    assert R.cast_rows([1, 300], [True, False], "i32", "i8") == ([1, 0], [True, False], None)
    for src in R.ALL:
        for dst in R.ALL:
            if R.supported(src, dst) and not R.can_fail(src, dst):
                assert not R.failing_rows(src, dst), (src, dst)
            elif R.supported(src, dst):
                assert R.failing_rows(src, dst) and R.clean_rows(src, dst), (src, dst)


# ---- grammar ------------------------------------------------------------------------------------------------------------
X = A.ident("a")
TYPE_NAMES = {"boolean": "Boolean", "BOOL": "Boolean", "tinyint": "Int8", "SmallInt": "Int16", "int": "Int32", "INTEGER": "Int32", "bigint": "Int64",
              "tinyint unsigned": "UInt8", "smallint UNSIGNED": "UInt16", "int unsigned": "UInt32", "integer unsigned": "UInt32",
              "bigint unsigned": "UInt64", "real": "Float32", "FLOAT": "Float32", "double": "Float64", "double precision": "Float64",
              "varchar": "Utf8", "TEXT": "Utf8", "string": "Utf8"}


def test_grammar_three_spellings_and_every_type_name():
    for name, typ in TYPE_NAMES.items():
        to = A.CastType[typ]
        assert parse_expr(f"cast(a as {name})") == A.Cast(X, to, False) == parse_expr(f"CAST(a AS {name})") == parse_expr(f"a::{name}"), name
        assert parse_expr(f"try_cast(a as {name})") == A.Cast(X, to, True) == parse_expr(f"TRY_CAST(a AS {name})"), name
    assert [int(A.CastType[n]) for n in R.NAME.values()] == [R.CODE[k] for k in R.NAME]      # the numbers of include/chq.h
    header = open(os.path.join(ROOT, "include", "chq.h")).read()
    enum = re.search(r"typedef enum chq_cast_type \{(.*?)\}", header, re.S).group(1)
    names = [n.strip().split("=")[0].strip() for n in enum.split(",")]
    assert names == ["CHQ_CAST_BOOLEAN", "CHQ_CAST_INT8", "CHQ_CAST_INT16", "CHQ_CAST_INT32", "CHQ_CAST_INT64", "CHQ_CAST_UINT8", "CHQ_CAST_UINT16",
                     "CHQ_CAST_UINT32", "CHQ_CAST_UINT64", "CHQ_CAST_FLOAT16", "CHQ_CAST_FLOAT32", "CHQ_CAST_FLOAT64", "CHQ_CAST_UTF8", "CHQ_CAST_OTHER"]
    assert [m.name.upper() for m in A.CastType] == [n[len("CHQ_CAST_"):] for n in names]


def test_grammar_binding_and_aliases():
    B, Op = A.BinaryOp, A.BinaryOperator
    i32 = A.CastType.Int32
    assert parse_expr("a::int * 2") == B(A.Cast(X, i32), Op.Multiply, A.number("2"))
    assert parse_expr("2 * a::int") == B(A.number("2"), Op.Multiply, A.Cast(X, i32))
    assert parse_expr("a + b::bigint > 1") == B(B(X, Op.Plus, A.Cast(A.ident("b"), A.CastType.Int64)), Op.Gt, A.number("1"))
    assert parse_expr("a::int::varchar") == A.Cast(A.Cast(X, i32), A.CastType.Utf8)
    assert parse_expr("(a + 1)::int") == A.Cast(A.Nested(B(X, Op.Plus, A.number("1"))), i32)
    assert parse_expr("cast(a + 1 as int)") == A.Cast(B(X, Op.Plus, A.number("1")), i32)
    assert parse_expr("cast(cast(a as varchar) || 'x' as text)") == A.Cast(B(A.Cast(X, A.CastType.Utf8), Op.StringConcat, A.string("x")), A.CastType.Utf8)
    assert parse_expr("s::int is null") == A.IsNull(A.Cast(A.ident("s"), i32), False)
    sel = parse_select("select cast(a as int) as b, try_cast(a as varchar) c, a::bigint d, cast(a as int) from read_files('x') where cast(a as int) > 100")
    assert sel.projection[0] == A.ExprWithAlias(A.Cast(X, i32), A.Ident("b"))
    assert sel.projection[1] == A.ExprWithAlias(A.Cast(X, A.CastType.Utf8, True), A.Ident("c"))
    assert sel.projection[2] == A.ExprWithAlias(A.Cast(X, A.CastType.Int64), A.Ident("d"))
    assert sel.projection[3] == A.UnnamedExpr(A.Cast(X, i32))
    assert sel.selection == B(A.Cast(X, i32), Op.Gt, A.number("100"))
    # `cast` and `try_cast` stay ordinary words where no parenthesis follows
    assert parse_expr("cast + 1") == B(A.ident("cast"), Op.Plus, A.number("1"))
    assert parse_select("select a cast from read_files('x')").projection[0] == A.ExprWithAlias(X, A.Ident("cast"))


@pytest.mark.parametrize("sql", ["cast(a as varchar(10))", "cast(a as float(24))", "a::varchar(3)", "cast(a as date)", "cast(a as timestamp)",
                                 "cast(a as decimal)", "a::numeric", "cast(a as unsigned)", "cast(a int)", "cast(a as)", "try_cast(a as blob)",
                                 "cast(a as real unsigned)", "a::"])
def test_grammar_refusals(sql):
    with pytest.raises(SqlParseError):
        parse_expr(sql)


# ---- the library's host half ------------------------------------------------------------------------------------------------
SCHEMA = pa.schema([("s", pa.utf8()), ("id", pa.int32()), ("b", pa.bool_()), ("t", pa.utf8()), ("big", pa.int64()), ("u8", pa.uint8()),
                    ("f", pa.float32()), ("g", pa.float64()), ("h", pa.float16()), ("d", pa.date32()), ("ts", pa.timestamp("s")),
                    ("dec", pa.decimal128(30, 2)), ("i8", pa.int8()), ("i16", pa.int16()), ("u16", pa.uint16()), ("u32", pa.uint32()),
                    ("u64", pa.uint64())])
COLUMN = {"bool": "b", "i8": "i8", "i16": "i16", "i32": "id", "i64": "big", "u8": "u8", "u16": "u16", "u32": "u32", "u64": "u64", "f16": "h",
          "f32": "f", "f64": "g", "utf8": "s"}


def describe(expr, rows=2):
    try:
        return 0, chq.plan_describe(SCHEMA, None, parse_expr(expr) if isinstance(expr, str) else expr, rows)
    except chq.ChqError as e:
        return e.code, str(e)


def cast_lines(expr):
    code, out = describe(expr)
    assert code == 0, (expr, out)
    lines = out.splitlines()
    assert lines[1].startswith("split "), (expr, out)
    return lines[0], lines[1], [ln[len("cast "):] for ln in lines[2:] if ln.startswith("cast ")]


def folded(sql):
    code, text = describe(sql)
    assert code == 0, (sql, text)
    head, _, rest = text.partition("\n")
    m = re.fullmatch(r"result (\w+) scalar=[01] len1=1", head)
    assert m, (sql, text)
    if m.group(1) == "Utf8":
        return "Utf8", rest[len("value '"):-2]
    return m.group(1), int(rest.split()[1], 16)


def test_every_pair_types_as_the_rules_say():
    for src in R.ALL:
        for dst in R.ALL:
            for try_cast in (False, True):
                expr = A.Cast(A.ident(COLUMN[src]), A.CastType(R.CODE[dst]), try_cast)
                code, out = describe(expr)
                if not R.supported(src, dst):
                    assert code == R.NOT_SUPPORTED and R.NAME[src] in out and R.NAME[dst] in out, (src, dst, out)
                elif src == dst:      # the operand itself: no node, no kernel
                    assert code == 0 and out.splitlines()[1] == f"column {SCHEMA.get_field_index(COLUMN[src])}", (src, dst, out)
                else:
                    head, split, casts = cast_lines(expr)
                    assert head == f"result {R.NAME[dst]} scalar=0 len1=0" and split == "split an explicit cast runs as its own kernel"
                    assert casts == [f"{R.NAME[src]} -> {R.NAME[dst]}" + (" try" if try_cast else "")], (src, dst, casts)


def test_out_of_scope_types():
    for col in ("d", "ts", "dec"):
        for to in (A.CastType.Int32, A.CastType.Utf8, A.CastType.Int64):
            assert describe(A.Cast(A.ident(col), to))[0] == R.NOT_SUPPORTED, (col, to)
    for col in ("id", "s", "f", "b"):
        assert describe(A.Cast(A.ident(col), A.CastType.Other))[0] == R.NOT_SUPPORTED
        assert describe(A.Cast(A.ident(col), A.CastType.Other, True))[0] == R.NOT_SUPPORTED
    assert describe("cast(f as varchar)")[0] == R.NOT_SUPPORTED == describe("cast(s as double)")[0] == describe("try_cast('1.5' as real)")[0]
    # the operand is typed first: its error wins over the target's
    assert describe("cast(nope as int)")[0] == describe("nope")[0] != 0 and describe(A.Cast(A.ident("nope"), A.CastType.Other))[0] == describe("nope")[0]


def test_literal_folds():
    assert folded("cast('12' as int)") == ("Int32", 12) and folded("cast(1.9 as int)") == ("Int32", 1) and folded("'007'::bigint") == ("Int64", 7)
    assert folded("cast('-5' as int)") == ("Int32", 2**64 - 5) and folded("cast('-5' as tinyint)") == ("Int8", 2**64 - 5)
    assert folded("try_cast('x' as int) is null") == ("Boolean", 1) and folded("try_cast('12' as int) is null") == ("Boolean", 0)
    assert folded("try_cast(300 as tinyint) is null") == ("Boolean", 1) and folded("try_cast('-1' as int unsigned) is null") == ("Boolean", 1)
    assert folded("cast(12 as varchar)") == ("Utf8", "12") and folded("cast('-12' as int)::varchar") == ("Utf8", "-12")
    assert folded("cast(true as varchar) || cast(1 > 2 as text)") == ("Utf8", "truefalse")
    assert folded("cast(true as double)") == ("Float64", F.encode(0, 1, "f64")) and folded("cast(3 as real)") == ("Float32", F.encode(0, 3, "f32"))
    assert folded("cast(16777217 as real)") == ("Float32", F.encode(0, 16777216, "f32")) and folded("cast(1.5 as double)") == ("Float64", F.encode(0, 1.5, "f64"))
    assert folded("cast('yes' as boolean)") == ("Boolean", 1) and folded("cast(0 as boolean)") == ("Boolean", 0) and folded("cast(0.5 as boolean)") == ("Boolean", 1)
    assert folded("cast(3000000000 as int unsigned)") == ("UInt32", 3000000000) and folded("cast(255 as tinyint unsigned)") == ("UInt8", 255)
    assert folded(A.Cast(A.number("65520"), A.CastType.Float16)) == ("Float16", 0x7C00) and folded(A.Cast(A.number("65519"), A.CastType.Float16)) == ("Float16", 0x7BFF)
    assert folded("cast(12 as int)") == ("Int32", 12)      # the operand itself
    # the device's rules on every string edge, folded
    for dst in ("i32", "u8", "i64"):
        for s in R.string_edges():
            if b"'" in s or b"\x00" in s:
                continue
            lit = "'" + s.decode() + "'"
            want = R.cast_value(s, "utf8", dst)
            code, out = describe(f"cast({lit} as {R.SQL[dst]})")
            if want is R.FAIL:
                assert code == R.CAST_ERROR and "Utf8" in out and R.NAME[dst] in out, (s, dst, out)
                assert folded(f"try_cast({lit} as {R.SQL[dst]}) is null") == ("Boolean", 1), (s, dst)
            else:
                assert folded(f"cast({lit} as {R.SQL[dst]})") == (R.NAME[dst], want % 2**64), (s, dst)


def test_failing_literal_cast_fails_at_typing_wherever_it_stands():
    for sql in ("cast('x' as int)", "id + cast('x' as int)", "case when id > 0 then 1 else cast('x' as int) end", "cast(300 as tinyint) > i8",
                "coalesce(id, cast('' as int))", "cast(1.5 as double)::varchar is null or cast('q' as boolean)"):
        code, out = describe(sql)
        assert code in (R.CAST_ERROR, R.NOT_SUPPORTED), (sql, out)
    assert describe("case when id > 0 then 1 else cast('x' as int) end")[0] == R.CAST_ERROR
    assert describe("case when id > 0 then 1 else try_cast('x' as int) end")[0] == 0


def test_composition():
    head, split, casts = cast_lines("cast(id as bigint) * 1000000")
    assert head == "result Int64 scalar=0 len1=0" and casts == ["Int32 -> Int64"]
    assert cast_lines("cast(s as int) > 5")[::2] == ("result Boolean scalar=0 len1=0", ["Utf8 -> Int32"])
    code, out = describe("cast(id as varchar) || '-' || s")
    assert code == 0 and out.splitlines()[0] == "result Utf8 scalar=0 len1=0" and "strfn concat parts=3" in out and "cast Int32 -> Utf8" in out
    code, out = describe("upper(cast(b as varchar))")
    assert code == 0 and "strfn upper" in out and "cast Boolean -> Utf8" in out
    assert cast_lines("cast(id as varchar) like '1%'")[2] == ["Int32 -> Utf8"] and cast_lines("cast(id as varchar) = '5'")[2] == ["Int32 -> Utf8"]
    assert cast_lines("length(big::varchar) + id::bigint")[2] == ["Int64 -> Utf8", "Int32 -> Int64"]
    assert cast_lines("cast(cast(s as int) as bigint)")[2] == ["Utf8 -> Int32", "Int32 -> Int64"]      # operands first
    assert describe("cast(id as varchar) + 1")[0] != 0 and describe("cast(id as bigint) || 'x'")[0] == 22
    # a cast result as a CASE branch; a CAST that can fail is guarded, a TRY_CAST or an infallible CAST is not
    code, out = describe("case when s like '0%' then 0 else cast(s as int) end")
    assert code == 0 and "case whens=1 else=1 type=Int32 guarded=1" in out and "cast Utf8 -> Int32" in out
    assert "guarded=0" in describe("case when s like '0%' then 0 else try_cast(s as int) end")[1]
    assert "guarded=0" in describe("case when id > 0 then cast(id as bigint) else big end")[1]
    assert "guarded=1" in describe("case when id > 0 then cast(big as int) else id end")[1]
    assert "guarded=1" in describe("case when id > 0 then cast(f as int) else id end")[1]
    assert "guarded=0" in describe("case when id > 0 then cast(id as double) else g end")[1]
    code, out = describe("coalesce(try_cast(s as int), cast('-1' as int))")
    assert code == 0 and "type=Int32" in out and "cast Utf8 -> Int32 try" in out
    # is_scalar / len1 follow the operand
    assert describe("cast(1 as bigint)")[1].startswith("result Int64 scalar=1 len1=1")


# ---- the per-row rules alone, under the sanitizers ---------------------------------------------------------------------------
def bits64(v, typ):
    """the 64-bit form of cast_device.h"""
    if typ == "bool":
        return int(v)
    return v % 2**64


def narrowed(v, typ):
    if typ == "bool":
        return int(v)
    width = F.FORMATS[typ].width if typ in R.FLOATS else I.TYPES[typ].width
    return v % 2**width


def hexed(b):
    return b.hex() if b else "-"


def sanitizer_cases():
    lines = []
    for src in R.FIXED:
        for dst in R.FIXED:
            if src == dst:
                continue
            for v in R.edges(src):
                want = R.cast_value(v, src, dst)
                lines.append(f"fixed {R.CODE[src]} {R.CODE[dst]} {bits64(v, src)} {'fail' if want is R.FAIL else narrowed(want, dst)}")
    for dst in R.INTS:
        for s in R.string_edges() + [b"9" * 300, b"0" * 300 + b"1"]:
            want = R.cast_value(s, "utf8", dst)
            lines.append(f"parse 12 {R.CODE[dst]} {hexed(s)} {'fail' if want is R.FAIL else narrowed(want, dst)}")
    for src in ("bool",) + R.INTS:
        for v in R.edges(src):
            lines.append(f"print {R.CODE[src]} 12 {bits64(v, src)} {hexed(R.cast_value(v, src, 'utf8'))}")
    return lines


def test_row_functions_under_host_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler on PATH")
    exe = str(tmp_path / "cast_main")
    flags = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    src = os.path.join(ROOT, "tests", "cast_main.cpp")
    # the runtimes linked statically where the compiler has them that way: the program then needs nothing from its environment
    build = subprocess.run([cxx, *flags, "-static-libasan", "-static-libubsan", src, "-o", exe], capture_output=True, text=True)
    if build.returncode != 0:
        build = subprocess.run([cxx, *flags, src, "-o", exe], capture_output=True, text=True)
    if build.returncode != 0 and re.search(r"asan|ubsan|sanitize", build.stderr, re.I):
        pytest.skip("the compiler has no sanitizer runtime: " + build.stderr.strip().splitlines()[-1])
    assert build.returncode == 0, build.stderr
    lines = sanitizer_cases()
    assert len(lines) > 10000
    cases = tmp_path / "cases.txt"
    cases.write_text("\n".join(lines) + "\n")
    run = subprocess.run([exe, str(cases)], capture_output=True, text=True)
    if run.returncode != 0 and "runtime does not come first" in run.stderr:
        pytest.skip("this environment preloads a library in front of the sanitizer runtime: " + run.stderr.strip().splitlines()[0])
    assert run.returncode == 0, run.stdout + run.stderr[-4000:]
    assert run.stdout.startswith(f"{len(lines)} cases, 0 mismatches"), run.stdout


# ---- the round sizes of tests/test_gpu_cast.py, held to the sources -----------------------------------------------------------
def test_round_sizes_of_the_gpu_tests():
    from . import test_gpu_cast as G
    header = open(os.path.join(CSRC, "cast_device.h")).read()
    kernels = open(os.path.join(CSRC, "cast.hip")).read()
    const = lambda name: int(eval(re.search(r"constexpr\s+int\s+" + name + r"\s*=\s*([\d *]+);", header).group(1)))
    cap, block = const("CAST_GRID_CAP"), const("CAST_BLOCK")
    # every launch of cast.hip goes through rows_grid (typed_ops.h): capped at CAST_GRID_CAP workgroups of CAST_BLOCK threads, a
    # row per thread.  The clamp and the round loop are the shared ones, written for workgroups of kRowsBlock = CAST_BLOCK threads.
    shared, grid = (open(os.path.join(CSRC, name)).read() for name in ("wave_rows.h", "typed_ops.h"))
    assert "static_assert(CAST_BLOCK == kRowsBlock," in kernels and f"constexpr int kRowsBlock = {block};" in shared
    assert grid.count("inline unsigned rows_grid(int64_t items, int64_t cap_blocks) {") == 1 and f"blocks = (items + {block - 1}) / {block};" in grid
    assert grid.count("blocks < 1 ? 1 : blocks > cap_blocks ? cap_blocks : blocks") == 1 and "blocks >" not in kernels
    launches = re.findall(r"hipLaunchKernelGGL\((.*?), (dim3\(.*?\)|grid), (dim3\(.*?\)|block), 0, stream, p\)", kernels)
    assert len(launches) == 6 == kernels.count("hipLaunchKernelGGL(")
    assert all(g in ("dim3(rows_grid(p.nrows, CAST_GRID_CAP))", "grid") and b in ("dim3(CAST_BLOCK)", "block") for _, g, b in launches), launches
    assert "const dim3 grid(rows_grid(p.nrows, CAST_GRID_CAP)), block(CAST_BLOCK);" in kernels
    assert kernels.count("CHQ_FOR_WAVE_ROWS(base, p.nrows) {") == 3 and shared.count("base += (int64_t)gridDim.x * kRowsBlock)") == 1
    assert kernels.count("gridDim") == 1 and kernels.count("+= (int64_t)gridDim.x * CAST_BLOCK") == 1   # (cast_write_kernel: a lane per row, no ballot)
    assert kernels.count("__launch_bounds__(CAST_BLOCK)") == 4
    assert G.GRID_ROWS == cap * block
    # the offsets scan of integer -> Utf8: tiles of STRFN_SCAN_CHUNK rows, one tile total per thread of one workgroup and round
    strfn = open(os.path.join(CSRC, "strfn_device.h")).read()
    scan = open(os.path.join(CSRC, "scan_device.h")).read()
    tile = int(re.search(r"constexpr\s+int\s+STRFN_SCAN_CHUNK\s*=\s*(\d+);", strfn).group(1))
    scan_block = int(re.search(r"constexpr\s+int\s+kScanBlock\s*=\s*(\d+);", scan).group(1))
    assert G.SCAN_TILE == tile and G.SCAN_ROUND == tile * scan_block
    # (written once, in the Utf8 assembly every operator with a Utf8 result goes through)
    host = open(os.path.join(CSRC, "materialize.cpp")).read()
    body = lambda head: host.split("\n" + head)[1].split("\n}\n")[0]
    formula = "STRFN_SCAN_CHUNK - 1) / STRFN_SCAN_CHUNK"
    assert host.count(formula) == 1 and formula in body("void assemble_utf8(")
    for caller in ("Column evaluate_cast(", "Column evaluate_strfn(", "Column evaluate_case("):
        assert host.count(caller) == 1 and "assemble_utf8(ctx, c, " in body(caller), caller
    # the GPU tests' sizes: the scan tile and its neighbours, and the smallest count whose last word lies in the second round
    assert set(G.ROW_COUNTS) >= {0, 1, 63, 64, 65, tile - 1, tile, tile + 1}
    assert G.SECOND_ROUND_ROWS == G.GRID_ROWS + 1 and G.SECOND_ROUND_ROWS > G.SCAN_ROUND + tile
