"""CPU: CASE, COALESCE, NULLIF, BETWEEN and IN lists without a GPU.  The tests' reference (tests/case_reference.py) against
sqlite3 and pyarrow.compute; the grammar; the library's host half (typing, result types, status codes, constant folding, the
`case` line of a plan description, nesting, the desugaring of BETWEEN and IN) through `chq_plan_describe`; and the rules of
case_device.h alone in a stand-alone program under the address and undefined-behaviour sanitizers."""
import decimal
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

from . import case_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_HDR = open(os.path.join(ROOT, "chapterhouseqe_amd", "csrc", "case_device.h")).read()
MAX_WHENS = int(re.search(r"CASE_MAX_WHENS\s*=\s*(\d+)", _HDR).group(1))
MAX_IN = int(re.search(r"CASE_MAX_IN_LIST\s*=\s*(\d+)", _HDR).group(1))
INVALID_ARGUMENT, NOT_SUPPORTED, COERSION, DIV_ZERO, OVERFLOW = 22, 30, 9, 21, 20

# ---- a fixed table: every type family, nulls in conditions and values ------------------------------------------------------
N = 24
D = decimal.Decimal
C1 = [None if i % 5 == 3 else i % 3 == 0 for i in range(N)]
C2 = [None if i % 7 == 2 else i % 2 == 0 for i in range(N)]
C3 = [i % 4 == 1 for i in range(N)]


def nulled(vals, step, at):
    return [None if i % step == at else v for i, v in enumerate(vals)]


FAMILIES = {   # name -> (arrow type, column a, column b, a literal of the type or None)
    "Int8": (pa.int8(), nulled([i - 12 for i in range(N)], 6, 1), nulled([100 - i for i in range(N)], 3, 1), 7),
    "Int16": (pa.int16(), nulled([i * 1000 - 12000 for i in range(N)], 6, 1), nulled([30000 - i for i in range(N)], 3, 1), 7),
    "Int32": (pa.int32(), nulled([i * 10**8 - 12 * 10**8 for i in range(N)], 6, 1), nulled([2**31 - 1 - i for i in range(N)], 3, 1), 7),
    "Int64": (pa.int64(), nulled([i * 10**17 - 12 * 10**17 for i in range(N)], 6, 1), nulled([2**63 - 1 - i for i in range(N)], 3, 1), 3000000000),
    "UInt8": (pa.uint8(), nulled([i * 10 for i in range(N)], 6, 1), nulled([255 - i for i in range(N)], 3, 1), None),
    "UInt32": (pa.uint32(), nulled([i * 10**8 for i in range(N)], 6, 1), nulled([2**32 - 1 - i for i in range(N)], 3, 1), None),
    "UInt64": (pa.uint64(), nulled([i * 10**17 for i in range(N)], 6, 1), nulled([2**63 + i for i in range(N)], 3, 1), None),
    "Float32": (pa.float32(), nulled([i * 0.5 - 3 for i in range(N)], 6, 1), nulled([1.0 / (i + 1) for i in range(N)], 3, 1), 1.5),
    "Float64": (pa.float64(), nulled([i * 0.1 - 1 for i in range(N)], 6, 1), nulled([1e300 / (i + 1) for i in range(N)], 3, 1), None),
    "Boolean": (pa.bool_(), nulled([i % 2 == 0 for i in range(N)], 6, 1), nulled([i % 3 == 0 for i in range(N)], 3, 1), True),
    "Utf8": (pa.utf8(), nulled(["", "a", "héllo", "日本語", "x" * 40][0:5] * 5, 6, 1)[:N], nulled([f"b{i}" for i in range(N)], 3, 1), "lit"),
    "Date32": (pa.date32(), nulled(list(range(19000, 19000 + N)), 6, 1), nulled(list(range(-5, N - 5)), 3, 1), None),
    "Timestamp(s)": (pa.timestamp("s"), nulled([2**40 + i for i in range(N)], 6, 1), nulled([-2**40 + i for i in range(N)], 3, 1), None),
    "Decimal128(30,2)": (pa.decimal128(30, 2), nulled([D(2**70 + i) / 100 for i in range(N)], 6, 1), nulled([D(-i) / 100 for i in range(N)], 3, 1), None),
}
assert all(len(f[1]) == N and len(f[2]) == N for f in FAMILIES.values())


def f32(vals):
    return [None if v is None else float(np.float32(v)) for v in vals]


def column(name, which):
    typ, a, b, _ = FAMILIES[name]
    vals = (a, b)[which]
    return f32(vals) if name == "Float32" else vals


def arrow(name, vals):
    return pa.array(vals, FAMILIES[name][0])


def plain(arr):
    """to_pylist, with dates and timestamps as the integers they were built from"""
    if pa.types.is_date32(arr.type):
        arr = arr.cast(pa.int32())
    elif pa.types.is_timestamp(arr.type):
        arr = arr.cast(pa.int64())
    return arr.to_pylist()


# ---- the reference against two independent implementations -------------------------------------------------------------------
@pytest.mark.parametrize("name", list(FAMILIES))
def test_reference_agrees_with_pyarrow(name):
    a, b = column(name, 0), column(name, 1)
    conds = pa.StructArray.from_arrays([pa.array(C1, pa.bool_()), pa.array(C2, pa.bool_()), pa.array(C3, pa.bool_())], names=["c1", "c2", "c3"])
    # three WHENs with an ELSE, without one, and one WHEN
    assert plain(pc.case_when(conds, arrow(name, a), arrow(name, b), arrow(name, a), arrow(name, b))) == R.case_when([C1, C2, C3], [a, b, a], b)
    assert plain(pc.case_when(conds, arrow(name, a), arrow(name, b), arrow(name, a))) == R.case_when([C1, C2, C3], [a, b, a])
    one = pa.StructArray.from_arrays([pa.array(C1, pa.bool_())], names=["c"])
    assert plain(pc.case_when(one, arrow(name, a), arrow(name, b))) == R.case_when([C1], [a], b)
    # a searched CASE with one WHEN and an ELSE is if_else with a null condition read as false
    assert plain(pc.if_else(pc.fill_null(pa.array(C2, pa.bool_()), False), arrow(name, b), arrow(name, a))) == R.case_when([C2], [b], a)
    assert plain(pc.coalesce(arrow(name, a), arrow(name, b))) == R.coalesce(a, b)
    assert plain(pc.coalesce(arrow(name, a), arrow(name, b), arrow(name, a[::-1]))) == R.coalesce(a, b, a[::-1])
    assert sum(v is None for v in R.coalesce(a, b)) > 0 and sum(v is None for v in R.case_when([C1, C2, C3], [a, b, a])) > N // 8
    # nullif(a, b) = if_else(a = b, null, a) with a null comparison read as false
    eq = pc.fill_null(pc.equal(arrow(name, a), arrow(name, a[:5] + b[5:])), False)
    assert plain(pc.if_else(eq, pa.nulls(N, FAMILIES[name][0]), arrow(name, a))) == R.nullif(a, a[:5] + b[5:])


def _sqlite_value(name, v):
    if v is None:
        return None
    if name == "Boolean":
        return int(v)
    if name.startswith("Decimal"):
        return str(v)
    if name == "UInt64":
        return str(v)      # past sqlite's integers: compared as text, equality is all CASE needs
    return v


@pytest.mark.parametrize("name", list(FAMILIES))
def test_reference_agrees_with_sqlite(name):
    a, b = column(name, 0), column(name, 1)
    db = sqlite3.connect(":memory:")
    db.execute("create table t (i integer, c1, c2, c3, a, b)")
    conv = lambda vals: [_sqlite_value(name, v) for v in vals]
    db.executemany("insert into t values (?, ?, ?, ?, ?, ?)", list(zip(range(N), conv_bool(C1), conv_bool(C2), conv_bool(C3), conv(a), conv(b))))
    col = lambda sql: [r[0] for r in db.execute(f"select {sql} from t order by i")]
    assert col("case when c1 then a when c2 then b when c3 then a else b end") == conv(R.case_when([C1, C2, C3], [a, b, a], b))
    assert col("case when c1 then a when c2 then b end") == conv(R.case_when([C1, C2], [a, b]))
    assert col("coalesce(a, b)") == conv(R.coalesce(a, b))
    mixed = a[:5] + b[5:]
    db.execute("create table u (i integer, a, m)")
    db.executemany("insert into u values (?, ?, ?)", list(zip(range(N), conv(a), conv(mixed))))
    assert [r[0] for r in db.execute("select nullif(a, m) from u order by i")] == conv(R.nullif(a, mixed))
    assert [r[0] for r in db.execute("select case a when m then 1 else 0 end from u order by i")] == R.simple_case(a, [mixed], [[1] * N], [0] * N)


def conv_bool(vals):
    return [None if v is None else int(v) for v in vals]


def test_reference_sugar_agrees_with_sqlite_where_nothing_is_null():
    """BETWEEN and IN are typed as chains of the library's own AND / OR (null when either side is): sqlite's are Kleene's, so the
    pin holds on rows without a null operand, and on every row of a chain whose items are literals when x is valid"""
    x = [i - 8 for i in range(N)]
    lo = [(i * 3) % 7 - 3 for i in range(N)]
    hi = [(i * 5) % 11 for i in range(N)]
    db = sqlite3.connect(":memory:")
    db.execute("create table t (i integer, x, lo, hi)")
    db.executemany("insert into t values (?, ?, ?, ?)", list(zip(range(N), x, lo, hi)))
    col = lambda sql: [None if r[0] is None else bool(r[0]) for r in db.execute(f"select {sql} from t order by i")]
    assert col("x between lo and hi") == R.between(x, lo, hi) and col("x not between lo and hi") == R.between(x, lo, hi, True)
    assert col("x in (1, 3, -2)") == R.in_list(x, [1, 3, -2]) and col("x not in (1, 3, -2)") == R.in_list(x, [1, 3, -2], True)
    assert col(R.between_sql("x", "lo", "hi")) == R.between(x, lo, hi) and col(R.in_list_sql("x", [1, 3, -2], True)) == R.in_list(x, [1, 3, -2], True)
    assert R.between([None, 1], [0, None], [2, 2]) == [None, None] and R.in_list([None, 1], [1, 2]) == [None, True]


def test_reference_typing_and_lazy_rule():
    assert R.result_type(["Int8", "Int32", "Float32"]) == "Float32" and R.result_type(["UInt8", "Int16"]) == "Int16" and R.result_type(["Float16", "Float64"]) == "Float64"
    for a, b in (("Utf8", "Int32"), ("Boolean", "Int8"), ("Int64", "Float32"), ("UInt64", "Int64"), ("Int8", "UInt8"), ("Date32", "Timestamp(s)"), ("Float16", "Int8"),
                 ("Decimal128(30,2)", "Decimal128(30,3)")):
        with pytest.raises(R.NoCommonType):
            R.common_type(a, b)
    a, b = [6, 7, 8, None, 10], [3, 0, 2, 0, None]
    div = lambda i: R.checked("/", a[i], b[i])
    nz = lambda i: None if b[i] is None else b[i] != 0
    assert R.lazy_case(5, [nz], [div], lambda i: 0) == [2, 0, 4, 0, 0]
    with pytest.raises(R.DivideByZero):
        R.lazy_case(5, [lambda i: True], [div])
    # a null earlier condition is not true: the next WHEN is evaluated there
    with pytest.raises(R.DivideByZero):
        R.lazy_case(5, [lambda i: None if i == 1 else False, lambda i: div(i) > 1], [lambda i: 1, lambda i: 2])
    assert R.lazy_case(5, [lambda i: b[i] == 0, lambda i: div(i) is not None and div(i) > 2], [lambda i: -1, lambda i: 9]) == [None, -1, 9, -1, None]
    with pytest.raises(R.Overflow):
        R.checked("*", 2**31 - 1, 2)
    assert R.checked("/", -7, 2) == -3 and R.checked("%", -7, 2) == -1


# ---- grammar -------------------------------------------------------------------------------------------------------------------
I, B, Op = A.ident, A.BinaryOp, A.BinaryOperator
n1, n2, n3 = A.number("1"), A.number("2"), A.number("3")


def test_grammar_case_forms():
    assert parse_expr("case when a then 1 end") == A.Case(None, (I("a"),), (n1,), None)
    assert parse_expr("CASE WHEN a THEN 1 ELSE 2 END") == A.Case(None, (I("a"),), (n1,), n2)
    assert parse_expr("case when a > 1 then 1 when b then 2 else 3 end") == A.Case(None, (B(I("a"), Op.Gt, n1), I("b")), (n1, n2), n3)
    assert parse_expr("case x when 1 then 'a' when 2 then 'b' end") == A.Case(I("x"), (n1, n2), (A.string("a"), A.string("b")), None)
    assert parse_expr("case x + 1 when 2 then 1 end") == A.Case(B(I("x"), Op.Plus, n1), (n2,), (n1,), None)
    # nesting, and CASE as an operand: a prefix expression like any other
    inner = A.Case(None, (I("b"),), (n1,), n2)
    assert parse_expr("case when a then case when b then 1 else 2 end else 3 end") == A.Case(None, (I("a"),), (inner,), n3)
    assert parse_expr("case when b then 1 else 2 end + 3") == B(inner, Op.Plus, n3)
    assert parse_expr("3 * case when b then 1 else 2 end > 1") == B(B(n3, Op.Multiply, inner), Op.Gt, n1)
    assert parse_expr("(case when b then 1 else 2 end)") == A.Nested(inner)
    assert parse_expr("case when a and b or c then 1 end").conditions[0] == B(B(I("a"), Op.And, I("b")), Op.Or, I("c"))
    assert parse_expr("coalesce(a, 1)") == A.Function("Function(coalesce)", "coalesce", (I("a"), n1), False, None)
    assert parse_expr("NULLIF(a, b)").name == "NULLIF"
    for bad in ("case end", "case when a end", "case when a then 1", "case when a then 1 else end", "case a then 1 end", "case when then 1 end"):
        with pytest.raises(SqlParseError):
            parse_expr(bad)
    # `case` stays an ordinary word where no CASE follows
    assert parse_expr("case = 1") == B(I("case"), Op.Eq, n1) and parse_expr('"case"') == A.Identifier(A.Ident("case", '"'))


def test_grammar_in_and_between():
    assert parse_expr("a in (1, 2)") == A.InList(I("a"), (n1, n2), False) and parse_expr("a NOT IN (1)") == A.InList(I("a"), (n1,), True)
    assert parse_expr("a between 1 and 2") == A.Between(I("a"), False, n1, n2) and parse_expr("a not between 1 and 2") == A.Between(I("a"), True, n1, n2)
    # the AND belongs to BETWEEN; the next one is the conjunction; bounds are parsed above the comparison operators
    assert parse_expr("a between 1 and 2 and b") == B(A.Between(I("a"), False, n1, n2), Op.And, I("b"))
    assert parse_expr("a between 1 + 1 and 2 * 3 or b") == B(A.Between(I("a"), False, B(n1, Op.Plus, n1), B(n2, Op.Multiply, n3)), Op.Or, I("b"))
    assert parse_expr("a + 1 between 1 and 2") == A.Between(B(I("a"), Op.Plus, n1), False, n1, n2)
    assert parse_expr("b and a in (1, 2) or c") == B(B(I("b"), Op.And, A.InList(I("a"), (n1, n2), False)), Op.Or, I("c"))
    assert parse_expr("a + 1 in (1)") == A.InList(B(I("a"), Op.Plus, n1), (n1,), False)
    assert parse_expr("a in ((1), 'x', true)") == A.InList(I("a"), (A.Nested(n1), A.string("x"), A.boolean(True)), False)
    assert parse_expr("case when a in (1) then 1 when a between 1 and 2 then 2 end").conditions == (A.InList(I("a"), (n1,), False), A.Between(I("a"), False, n1, n2))
    for bad in ("a between 1", "a between 1 or 2", "a in ()", "a in (1", "a in 1"):
        with pytest.raises(SqlParseError):
            parse_expr(bad)
    # `in` and `between` elsewhere are ordinary words
    assert parse_select("select a between from read_files('x')").projection[0] == A.ExprWithAlias(I("a"), A.Ident("between"))


def test_grammar_select_where_aliases_and_window_frames():
    sel = parse_select("select case when id > 1 then 'big' else 'small' end bucket, coalesce(v, 0) as v0 from read_files('x') "
                       "where case when a then b else c end and id in (1, 2) and v between 0 and 9")
    assert isinstance(sel.projection[0].expr, A.Case) and sel.projection[0].alias == A.Ident("bucket") and sel.projection[1].alias == A.Ident("v0")
    assert isinstance(sel.selection, A.BinaryOp) and isinstance(sel.selection.right, A.Between) and isinstance(sel.selection.left.right, A.InList)
    # WHEN, THEN, ELSE and END are no implicit aliases any more; quoted, or behind AS, they are names
    for word in ("when", "then", "else", "end"):
        with pytest.raises(SqlParseError):
            parse_select(f"select a {word} from read_files('x')")
        assert parse_select(f"select a as \"{word}\" from read_files('x')").projection[0].alias == A.Ident(word, '"')
        assert parse_select(f"select a as {word} from read_files('x')").projection[0].alias == A.Ident(word)
    assert parse_select('select "end" from read_files(\'x\')').projection[0] == A.UnnamedExpr(A.Identifier(A.Ident("end", '"')))
    # ROWS BETWEEN of a window frame is parsed where it was
    w = parse_select("select sum(a) over (partition by b order by c rows between unbounded preceding and current row) s from read_files('x')")
    assert w.projection[0].expr.over.frame == A.WindowFrame.ROWS_TO_CURRENT
    w = parse_select("select sum(a) over (order by c range between unbounded preceding and unbounded following) from read_files('x')")
    assert w.projection[0].expr.over.frame == A.WindowFrame.PARTITION


# ---- the library's host half ---------------------------------------------------------------------------------------------------
SCHEMA = pa.schema([("s", pa.utf8()), ("id", pa.int32()), ("b", pa.bool_()), ("t", pa.utf8()), ("l", pa.int64()), ("f", pa.float32()), ("g", pa.float64()),
                    ("i8", pa.int8()), ("i16", pa.int16()), ("u8", pa.uint8()), ("u16", pa.uint16()), ("u32", pa.uint32()), ("u64", pa.uint64()), ("h", pa.float16()),
                    ("d", pa.date32()), ("d2", pa.date32()), ("ts", pa.timestamp("s")), ("tms", pa.timestamp("ms")), ("dec", pa.decimal128(30, 2)),
                    ("dec2", pa.decimal128(30, 2)), ("dec3", pa.decimal128(30, 3)), ("c", pa.bool_())])
TYPE_OF = {"s": "Utf8", "id": "Int32", "b": "Boolean", "l": "Int64", "f": "Float32", "g": "Float64", "i8": "Int8", "i16": "Int16", "u8": "UInt8", "u16": "UInt16",
           "u32": "UInt32", "u64": "UInt64", "h": "Float16", "1": "Int32", "1.5": "Float32", "'x'": "Utf8", "true": "Boolean", "3000000000": "Int64"}


def describe(sql, rows=2):
    try:
        return 0, chq.plan_describe(SCHEMA, None, parse_expr(sql) if isinstance(sql, str) else sql, rows)
    except chq.ChqError as e:
        return e.code, str(e)


def case_lines(sql):
    """(first line, the `case ...` lines) of a plan description: one line per CASE of the tree, operands first"""
    code, out = describe(sql)
    assert code == 0, (sql, out)
    lines = out.splitlines()
    assert lines[1].startswith("split "), (sql, out)
    return lines[0], [ln[len("case "):] for ln in lines[2:] if ln.startswith("case ")]


def folded(sql):
    code, text = describe(sql)
    assert code == 0, (sql, text)
    head, _, rest = text.partition("\n")
    m = re.fullmatch(r"result (\w+) scalar=[01] len1=1", head)      # (AND / OR flag their result non-scalar, folded or not)
    assert m, (sql, text)
    if m.group(1) == "Utf8":
        return "Utf8", rest[len("value '"):-2]
    return m.group(1), int(rest.split()[1], 16)


def test_result_types_across_the_coercion_table():
    names = list(TYPE_OF)
    met = 0
    for x in names:
        for y in names:
            code, out = describe(f"case when b then {x} else {y} end")
            try:
                want = R.common_type(TYPE_OF[x], TYPE_OF[y])
            except R.NoCommonType:
                assert code == COERSION, (x, y, out)
                continue
            met += 1
            if x in ("1", "1.5", "'x'", "true", "3000000000") and y in ("1", "1.5", "'x'", "true", "3000000000"):
                continue   # (a column condition with literal branches: still a CASE, checked below)
            assert code == 0 and out.splitlines()[0] == f"result {want} scalar=0 len1=0", (x, y, out)
            assert out.splitlines()[2] == f"case whens=1 else=1 type={want} guarded=0", (x, y, out)
    assert met > 100
    # folded left to right over every result and the ELSE
    assert case_lines("case when b then i8 when c then id else f end")[0] == "result Float32 scalar=0 len1=0"
    assert case_lines("case when b then u8 when c then i16 when b then l end")[0] == "result Int64 scalar=0 len1=0"
    assert describe("case when b then i8 when c then u8 else l end")[0] == COERSION      # Int8 with UInt8 has no entry, whatever follows
    assert case_lines("case when b then 1 else 2 end") == ("result Int32 scalar=0 len1=0", ["whens=1 else=1 type=Int32 guarded=0"])
    # temporal and decimal: only with the same type, which the output keeps
    for x, y, ok in (("d", "d2", True), ("dec", "dec2", True), ("ts", "ts", True), ("d", "ts", False), ("ts", "tms", False), ("dec", "dec3", False), ("d", "id", False), ("dec", "g", False)):
        code, out = describe(f"case when b then {x} else {y} end")
        assert (code == 0 and "type=FixedWidth" in out) if ok else code == COERSION, (x, y, out)
    assert describe("coalesce(d, d2)")[0] == 0 and describe("nullif(dec, dec2)")[0] == 0 and describe("nullif(dec, dec3)")[0] == COERSION
    assert describe("case when b then d else d2 end = d")[0] == NOT_SUPPORTED      # an operator on such a result: out of scope


def test_conditions_must_be_boolean():
    for cond, found in (("id", "Int32"), ("s", "Utf8"), ("f", "Float32"), ("1", "Int32"), ("'true'", "Utf8"), ("id + 1", "Int32")):
        code, out = describe(f"case when b then 1 when {cond} then 2 end")
        assert code == INVALID_ARGUMENT and "WHEN 2" in out and found in out, (cond, out)
    code, out = describe("case when id then 1 end")
    assert code == INVALID_ARGUMENT and "WHEN 1" in out and "Int32" in out
    # a simple CASE compares by the rules of `=`, statuses included
    assert describe("case id when 1 then 'a' end")[0] == 0 and describe("case l when id then 1 end")[0] == 0
    assert describe("case id when 'a' then 1 end") == describe("id = 'a'") and describe("case id when 'a' then 1 end")[0] == COERSION
    assert describe("case nope when 1 then 1 end")[0] == describe("nope = 1")[0] != 0


def test_coalesce_and_nullif_typing():
    assert case_lines("coalesce(id, 0)") == ("result Int32 scalar=0 len1=0", ["whens=1 else=1 type=Int32 guarded=0"])
    assert case_lines("COALESCE(i8, id, g)") == ("result Float64 scalar=0 len1=0", ["whens=2 else=1 type=Float64 guarded=0"])
    assert case_lines("Coalesce(s, t, 'none')")[0] == "result Utf8 scalar=0 len1=0"
    assert describe("coalesce(id)") == describe("id")      # one argument: the argument
    assert case_lines("nullif(id, 0)") == ("result Int32 scalar=0 len1=0", ["whens=1 else=1 type=Int32 guarded=0"])
    assert case_lines("NullIf(i8, l)")[0] == "result Int8 scalar=0 len1=0"      # a's own type, whatever the comparison widened to
    assert case_lines("nullif(s, 'x')")[0] == "result Utf8 scalar=0 len1=0" and case_lines("nullif(b, true)")[0] == "result Boolean scalar=0 len1=0"
    for text in ("coalesce()", "nullif()", "nullif(id)", "nullif(id, 1, 2)"):
        code, out = describe(text)
        assert code == INVALID_ARGUMENT and "argument" in out, (text, out)
    assert describe("coalesce(id, s)")[0] == COERSION and describe("nullif(id, s)")[0] == COERSION
    assert describe("coalesce(nope, 1)")[0] == describe("nope")[0] != 0


def test_literal_only_forms_fold():
    assert folded("case when 1 > 2 then 'a' else 'b' end") == ("Utf8", "b") and folded("case when 2 > 1 then 'a' else 'b' end") == ("Utf8", "a")
    assert folded("case when 1 > 2 then 1 when 2 > 1 then 2.5 else 3 end") == ("Float32", int(np.float32(2.5).view(np.uint32)))
    assert folded("case 3 when 1 then 10 when 3 then 30 else 0 end") == ("Int32", 30) and folded("case 'b' when 'a' then 1 when 'b' then 2 end") == ("Int32", 2)
    assert folded("coalesce(1, 2)") == ("Int32", 1) and folded("nullif(2, 1)") == ("Int32", 2) and folded("nullif('a', 'b')") == ("Utf8", "a")
    # null results: nullif of equals, no WHEN true without ELSE -- seen through IS NULL, which folds too
    assert folded("nullif(1, 1) is null") == ("Boolean", 1) and folded("nullif(2, 1) is null") == ("Boolean", 0)
    assert folded("case when 1 > 2 then 1 end is null") == ("Boolean", 1) and folded("coalesce(nullif(1, 1), 7)") == ("Int32", 7)
    assert folded("coalesce(nullif(1, 1), nullif(2, 2)) is null") == ("Boolean", 1)
    assert folded("case when nullif(true, true) then 1 else 2 end") == ("Int32", 2)      # a null condition is not true
    assert folded("1 between 0 and 2") == ("Boolean", 1) and folded("3 not between 0 and 2") == ("Boolean", 1) and folded("2 in (1, 2)") == ("Boolean", 1)
    assert folded("'b' in ('a', 'c')") == ("Boolean", 0) and folded("2 not in (1, 3)") == ("Boolean", 1)
    # a literal-only sub-expression folds at typing: its error is static, wherever it stands
    for text in ("case when b then 1 else 1 / 0 end", "case when 1 > 2 then 1 / 0 else 1 end", "coalesce(id, 1 / 0)", "case when id > 1 / 0 then 1 end"):
        assert describe(text)[0] == DIV_ZERO, text
    assert describe("case when b then 2147483647 + 1 end")[0] == OVERFLOW
    # is_scalar and len1 follow the operands: one column anywhere and it is a column
    for text in ("case when b then 1 else 2 end", "case when 1 > 2 then id else 2 end", "case when 1 > 2 then 1 else id end", "case id when 1 then 1 end"):
        assert describe(text)[1].splitlines()[0] == "result Int32 scalar=0 len1=0", text


def test_case_line_and_guards():
    assert case_lines("case when id <> 0 then l / id else 0 end")[1] == ["whens=1 else=1 type=Int64 guarded=1"]
    assert case_lines("case when id > 0 then id * 2 when id < 0 then id + 1 else id end")[1] == ["whens=2 else=1 type=Int32 guarded=2"]
    # the first condition is evaluated on every row: never guarded; later ones are
    assert case_lines("case when id / id > 0 then 1 end")[1] == ["whens=1 else=0 type=Int32 guarded=0"]
    assert case_lines("case when b then 1 when id / id > 0 then 2 end")[1] == ["whens=2 else=0 type=Int32 guarded=1"]
    # float arithmetic, comparisons, LIKE and string functions cannot fail: unguarded
    assert case_lines("case when f > 1.5 then f / 0.0 when s like 'a%' then g * g else length(s) end")[1] == ["whens=2 else=1 type=Float64 guarded=0"]
    assert case_lines("coalesce(l / id, 0)")[1] == ["whens=1 else=1 type=Int64 guarded=1"]
    # nested CASEs: one line each, operands first
    assert case_lines("case when b then case when c then 1 else 2 end else 3 end")[1] == ["whens=1 else=1 type=Int32 guarded=0", "whens=1 else=1 type=Int32 guarded=0"]
    assert case_lines("upper(case when b then s else t end) = 'A'")[1] == ["whens=1 else=1 type=Utf8 guarded=0"]
    assert case_lines("case when b then s end = 'a'")[1] == ["whens=1 else=0 type=Utf8 guarded=0"]
    assert case_lines("case when b then id end + 1 > 2")[1] == ["whens=1 else=0 type=Int32 guarded=0"]


def test_more_than_eight_whens_nest():
    assert MAX_WHENS == 8
    chain = lambda k, els="": "case " + " ".join(f"when id = {j} then {j * 10}" for j in range(k)) + els + " end"
    assert case_lines(chain(8))[1] == ["whens=8 else=0 type=Int32 guarded=0"]
    assert case_lines(chain(8, " else 1"))[1] == ["whens=8 else=1 type=Int32 guarded=0"]
    assert case_lines(chain(9))[1] == ["whens=1 else=0 type=Int32 guarded=0", "whens=8 else=1 type=Int32 guarded=0"]
    assert case_lines(chain(16, " else 1"))[1] == ["whens=8 else=1 type=Int32 guarded=0", "whens=8 else=1 type=Int32 guarded=0"]
    assert case_lines(chain(17))[1] == ["whens=1 else=0 type=Int32 guarded=0", "whens=8 else=1 type=Int32 guarded=0", "whens=8 else=1 type=Int32 guarded=0"]
    # the result type is common to every level
    assert case_lines(chain(9, " else g"))[1] == ["whens=1 else=1 type=Float64 guarded=0", "whens=8 else=1 type=Float64 guarded=0"]
    assert folded("case " + " ".join(f"when 9 = {j} then {j}" for j in range(12)) + " end") == ("Int32", 9)
    assert case_lines("coalesce(" + ", ".join(["id"] * 10) + ")")[1] == ["whens=1 else=1 type=Int32 guarded=0", "whens=8 else=1 type=Int32 guarded=0"]


def test_between_and_in_type_to_their_spelled_out_forms():
    for x, lo, hi in (("id", "1", "3"), ("id", "i8", "l"), ("f", "0.5", "id"), ("s", "'a'", "t"), ("id + 1", "1", "id * 2"), ("d", "d2", "d"), ("dec", "dec2", "dec2"),
                      ("id", "'a'", "3"), ("nope", "1", "2"), ("s", "1", "2"), ("h", "h", "f")):
        for neg in (False, True):
            sugar = f"{x} {'not ' if neg else ''}between {lo} and {hi}"
            assert describe(sugar) == describe(R.between_sql(x, lo, hi, neg)), sugar
    for x, items in (("id", ["1"]), ("id", ["1", "2", "3"]), ("l", ["1", "3000000000"]), ("f", ["1", "2.5"]), ("s", ["'a'", "'b'", "'c'"]), ("id + 1", ["(2)", "4"]),
                     ("b", ["true"]), ("id", ["'a'"]), ("nope", ["1"]), ("s", ["'a'"] * 5), ("id", [str(k) for k in range(MAX_IN)])):
        for neg in (False, True):
            sugar = f"{x} {'not ' if neg else ''}in ({', '.join(items)})"
            assert describe(sugar) == describe(R.in_list_sql(x, items, neg)), sugar
    assert describe("id between 1 and 3")[0] == 0 and describe("id in (1, 2)")[1].startswith("result Boolean scalar=0 len1=0\nprogram ")


def test_in_list_limits():
    assert MAX_IN == 32
    assert describe("id in (" + ", ".join(str(k) for k in range(MAX_IN)) + ")")[0] == 0
    code, out = describe("id in (" + ", ".join(str(k) for k in range(MAX_IN + 1)) + ")")
    assert code == NOT_SUPPORTED and "32" in out
    for text in ("id in (id)", "id in (1, id + 1)", "id in (1 + 1)", "s in (t)", "id in (coalesce(1, 2))", "id not in (l)"):
        code, out = describe(text)
        assert code == NOT_SUPPORTED and "literal" in out, (text, out)
    assert describe(A.InList(A.ident("id"), (), False))[0] == NOT_SUPPORTED
    # the limits are static: before the operand is looked up
    assert describe("nope in (id)")[0] == NOT_SUPPORTED


def test_expression_handles_own_their_children_on_failure():
    """the three constructors free every child when they refuse: nothing to free afterwards, nothing to crash on"""
    from chapterhouseqe_amd import _lib
    from chapterhouseqe_amd.record_utils import _expr_to_c
    import ctypes as C
    L = _lib.lib()
    one = lambda: _expr_to_c(parse_expr("id + 1"))
    assert not L.chq_expr_between(one(), 0, None, one())
    assert not L.chq_expr_in_list(None, (C.c_void_p * 1)(one()), 1, 0)
    assert not L.chq_expr_in_list(one(), (C.c_void_p * 2)(one(), None), 2, 0)
    assert not L.chq_expr_case(one(), (C.c_void_p * 1)(one()), (C.c_void_p * 1)(None), 1, one())
    assert not L.chq_expr_case(None, None, None, 0, one())
    h = L.chq_expr_case(None, (C.c_void_p * 1)(one()), (C.c_void_p * 1)(one()), 1, None)
    assert h
    L.chq_expr_free(h)
    with pytest.raises(ValueError):
        _expr_to_c(A.Case(None, (A.ident("b"),), (), None))


# ---- the rules of case_device.h alone, under the sanitizers --------------------------------------------------------------------
def test_case_rules_under_host_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler on PATH")
    exe = str(tmp_path / "case_main")
    flags = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    src = os.path.join(ROOT, "tests", "case_main.cpp")
    build = subprocess.run([cxx, *flags, "-static-libasan", "-static-libubsan", src, "-o", exe], capture_output=True, text=True)
    if build.returncode != 0:
        build = subprocess.run([cxx, *flags, src, "-o", exe], capture_output=True, text=True)
    if build.returncode != 0 and re.search(r"asan|ubsan|sanitize", build.stderr, re.I):
        pytest.skip("the compiler has no sanitizer runtime: " + build.stderr.strip().splitlines()[-1])
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe, "7"], capture_output=True, text=True)
    if run.returncode != 0 and "runtime does not come first" in run.stderr:
        pytest.skip("this environment preloads a library in front of the sanitizer runtime: " + run.stderr.strip().splitlines()[0])
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    m = re.fullmatch(r"(\d+) checks, 0 mismatches\n", run.stdout)
    assert m and int(m.group(1)) > 1000000, run.stdout
