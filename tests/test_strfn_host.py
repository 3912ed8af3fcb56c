"""CPU: the scalar string functions (`||`, upper / lower, length, octet_length, substring, trim) without a GPU.  The tests'
reference (tests/strfn_reference.py) against sqlite3 and pyarrow.compute; the grammar; the library's host half (typing, status
codes, constant folding with the per-row code the device runs) through `chq_plan_describe`; and that per-row code alone in a
stand-alone program under the address and undefined-behaviour sanitizers."""
import os
import re
import shutil
import sqlite3
import subprocess

import pyarrow as pa
import pyarrow.compute as pc
import pytest

import chapterhouseqe_amd as chq
from chapterhouseqe_amd import sqlast as A
from chapterhouseqe_amd.sqlparse import parse_expr, parse_select

from . import strfn_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_HDR = open(os.path.join(ROOT, "chapterhouseqe_amd", "csrc", "strfn_device.h")).read()
MAX_PARTS = int(re.search(r"STRFN_MAX_PARTS\s*=\s*(\d+)", _HDR).group(1))

STRINGS = R.CORNERS + R.random_strings()
WITH_NULLS = [None if i % 11 == 5 else s for i, s in enumerate(STRINGS)]


def as_bytes(values):
    return [None if v is None else v.encode() for v in values]


def as_text(values):
    return [None if v is None else v.decode() for v in values]


# ---- the reference against two independent implementations ------------------------------------------------------------------
def test_reference_agrees_with_pyarrow():
    arr = pa.array(WITH_NULLS, pa.utf8())
    raw = as_bytes(WITH_NULLS)
    assert len(raw) > 600
    assert pc.ascii_upper(arr).to_pylist() == as_text(R.over(R.upper, raw))
    assert pc.ascii_lower(arr).to_pylist() == as_text(R.over(R.lower, raw))
    assert pc.utf8_length(arr).to_pylist() == R.over(R.length, raw)
    assert pc.binary_length(arr).to_pylist() == R.over(R.octet_length, raw)
    assert pc.utf8_trim(arr, characters=" ").to_pylist() == as_text(R.over(R.trim, raw))
    assert pc.utf8_ltrim(arr, characters=" ").to_pylist() == as_text(R.over(R.ltrim, raw))
    assert pc.utf8_rtrim(arr, characters=" ").to_pylist() == as_text(R.over(R.rtrim, raw))
    other = pa.array([None if i % 7 == 3 else s for i, s in enumerate(reversed(STRINGS))], pa.utf8())
    want = [R.concat(a, b) for a, b in zip(raw, as_bytes(other.to_pylist()))]
    assert pc.binary_join_element_wise(arr, other, "").to_pylist() == as_text(want)
    assert sum(w is None for w in want) > len(want) // 8
    for p, n in R.WINDOWS:
        if p >= 1 and n is not None:
            assert pc.utf8_slice_codeunits(arr, p - 1, p - 1 + n).to_pylist() == as_text(R.over(R.substring, raw, p, n)), (p, n)
    # on invalid UTF-8, utf8_length also counts the bytes that are no continuation bytes
    bad = pa.array(R.INVALID, pa.binary()).view(pa.utf8())
    assert pc.utf8_length(bad).to_pylist() == [R.length(b) for b in R.INVALID]


def test_reference_agrees_with_sqlite():
    db = sqlite3.connect(":memory:")
    one = lambda sql, *args: db.execute(sql, args).fetchone()[0]
    for s in WITH_NULLS:
        b = None if s is None else s.encode()
        text = lambda v: None if v is None else v.decode()
        assert one("select upper(?)", s) == (None if s is None else text(R.upper(b))), s
        assert one("select lower(?)", s) == (None if s is None else text(R.lower(b))), s
        assert one("select length(?)", s) == (None if s is None else R.length(b)), s
        assert one("select trim(?)", s) == (None if s is None else text(R.trim(b))), s
        assert one("select ltrim(?)", s) == (None if s is None else text(R.ltrim(b))), s
        assert one("select rtrim(?)", s) == (None if s is None else text(R.rtrim(b))), s
    for i, s in enumerate(WITH_NULLS):
        o = WITH_NULLS[(i * 5 + 3) % len(WITH_NULLS)]
        assert one("select ? || ?", s, o) == text(R.concat(None if s is None else s.encode(), None if o is None else o.encode())), (s, o)
    for s in STRINGS[::3]:
        for p, n in R.WINDOWS:
            if p < 0:
                continue   # sqlite counts a negative position from the END: not a pin
            got = one("select substr(?, ?)", s, p) if n is None else one("select substr(?, ?, ?)", s, p, n)
            assert got == R.substring(s.encode(), p, n).decode(), (s, p, n)


def test_reference_corners():
    assert R.trim(b" \t a \t ") == b"\t a \t" and R.rtrim(b"a\t") == b"a\t"          # tabs stay
    assert R.upper("héllo ß".encode()) == "HéLLO ß".encode() and R.lower("ÀBC".encode()) == "Àbc".encode()   # ASCII only
    assert R.substring("héllo".encode(), 2, 3) == "éll".encode() and R.substring(b"abc", 0, 2) == b"a" and R.substring(b"abc", -1) == b"abc"
    # p <= 0: substring(s from p for n) = substring(s from 1 for max(0, p + n - 1)), on invalid rows too
    for s in as_bytes(STRINGS[:80]) + R.INVALID:
        for p in (-3, -1, 0):
            for n in (0, 1, 2, 3, 5, 100):
                assert R.substring(s, p, n) == R.substring(s, 1, max(0, p + n - 1)), (s, p, n)
            assert R.substring(s, p) == s
    assert R.length(b"\x80\x80a") == 1 and R.substring(b"\x80\x80ab", 2) == b"b" and R.substring(b"\x80\x80ab", 1, 1) == b"\x80\x80a"
    assert R.concat(b"a", None) is None and R.concat(b"a", b"", b"b") == b"ab"


# ---- grammar ------------------------------------------------------------------------------------------------------------
S = A.ident("s")


def fn(name, *args):
    return A.Function(f"Function({name})", name, tuple(args), False, None)


def test_grammar_substring_spellings():
    assert parse_expr("substring(s from 1 for 2)") == fn("substring", S, A.number("1"), A.number("2"))
    assert parse_expr("substring(s, 1, 2)") == fn("substring", S, A.number("1"), A.number("2"))
    assert parse_expr("substring(s from 2)") == fn("substring", S, A.number("2")) == parse_expr("substring(s, 2)")
    assert parse_expr("SUBSTRING(s FROM 1 FOR 2)") == fn("SUBSTRING", S, A.number("1"), A.number("2"))
    assert parse_expr("substr(s, 2, 3)") == fn("substr", S, A.number("2"), A.number("3"))
    assert parse_expr("substring(s from -3 for 5)") == fn("substring", S, A.number("-3"), A.number("5"))
    assert parse_expr("substr(s, -3)") == fn("substr", S, A.number("-3"))
    assert parse_expr("substring(s from (1) for id)") == fn("substring", S, A.Nested(A.number("1")), A.ident("id"))
    assert parse_expr("substring(upper(s) from 1 for 2) like 'A%'") == A.Like(fn("substring", fn("upper", S), A.number("1"), A.number("2")), A.string("A%"), False, None)
    assert parse_expr("substring(s from 1 for 2)").debug == "Function(substring)"


def test_grammar_names_and_concat():
    for name in ("upper", "UPPER", "Lower", "length", "CHAR_LENGTH", "character_length", "octet_length", "trim", "LTRIM", "rtrim"):
        assert parse_expr(f"{name}(s)") == fn(name, S)
    B, Op = A.BinaryOp, A.BinaryOperator
    assert parse_expr("s || 'x' || t") == B(B(S, Op.StringConcat, A.string("x")), Op.StringConcat, A.ident("t"))     # left-associative
    assert parse_expr("s || 'x' = t") == B(B(S, Op.StringConcat, A.string("x")), Op.Eq, A.ident("t"))
    assert parse_expr("upper(s) = 'AB' and length(s) > 3") == B(B(fn("upper", S), Op.Eq, A.string("AB")), Op.And, B(fn("length", S), Op.Gt, A.number("3")))
    sel = parse_select("select value1 || '-' || value1, upper(value1) u from read_files('x')")
    assert isinstance(sel.projection[0], A.UnnamedExpr) and sel.projection[1] == A.ExprWithAlias(fn("upper", A.ident("value1")), A.Ident("u"))


def test_grammar_other_calls_parse_as_before():
    assert parse_expr("abs(a)") == fn("abs", A.ident("a")) and repr(parse_expr("abs(a)")) == "UnsupportedExpr(debug='Function(abs)')"
    assert parse_expr("count(*)") == A.Function("Function(count)", "count", (), True, None)
    assert parse_expr("abs(a, -3)").args[1].debug.startswith("UnaryOp { op: Minus")
    assert parse_expr("trim(both 'x' from s)") == A.Function("Function(trim)", "trim", None, False, None)
    w = parse_expr("sum(a) over (partition by b order by c)")
    assert w.name == "sum" and w.args == (A.ident("a"),) and w.over is not None and w.over.partition_by == (A.ident("b"),)
    assert parse_expr("-abs(a)").debug == "UnaryOp { op: Minus, expr: UnsupportedExpr(debug='Function(abs)') }"


# ---- the library's host half ------------------------------------------------------------------------------------------------
SCHEMA = pa.schema([("s", pa.utf8()), ("id", pa.int32()), ("b", pa.bool_()), ("t", pa.utf8())])
UNARY = ["upper", "lower", "length", "char_length", "character_length", "octet_length", "trim", "ltrim", "rtrim"]
INT_FNS = {"length", "char_length", "character_length", "octet_length"}
INVALID_ARGUMENT, NOT_SUPPORTED = 22, 30


def describe(sql, rows=2):
    try:
        return 0, chq.plan_describe(SCHEMA, None, parse_expr(sql) if isinstance(sql, str) else sql, rows)
    except chq.ChqError as e:
        return e.code, str(e)


def folded(sql):
    """(result type, value) of a literal-only expression: a str for Utf8, an int otherwise"""
    code, text = describe(sql)
    assert code == 0, (sql, text)
    head, _, rest = text.partition("\n")
    m = re.fullmatch(r"result (\w+) scalar=1 len1=1", head)
    assert m, (sql, text)
    if m.group(1) == "Utf8":
        assert rest.startswith("value '") and rest.endswith("'\n"), (sql, text)
        return "Utf8", rest[len("value '"):-2]
    return m.group(1), int(rest.split()[1], 16)


@pytest.mark.parametrize("name", UNARY + ["substring", "substr"])
def test_typing_of_every_function(name):
    call = (lambda x, n=name: f"{n}({x}, 2, 3)") if name.startswith("subs") else (lambda x, n=name: f"{n}({x})")
    typ = "Int32" if name in INT_FNS else "Utf8"
    for text in (call("s"), call("s", name.upper()), call("s", name.capitalize()), call("(s)"), call("upper(s)"), call("s || t")):
        code, out = describe(text)
        assert code == 0 and out.splitlines()[0] == f"result {typ} scalar=0 len1=0" and out.splitlines()[1].startswith("split "), (text, out)
    code, out = describe(call("'aBc '"))
    assert code == 0 and out.splitlines()[0] == f"result {typ} scalar=1 len1=1", out
    for operand, found in (("id", "Int32"), ("b", "Boolean"), ("1", "Int32"), ("id > 1", "Boolean"), ("length(s)", "Int32")):
        code, out = describe(call(operand))
        assert code == INVALID_ARGUMENT and name in out and found in out, (name, operand, out)
    assert describe(call("nope"))[0] == describe("nope = 'a'")[0] != 0      # the operand's own errors come first


def test_arity():
    for name in UNARY:
        for text in (f"{name}()", f"{name}(s, s)", f"{name}(s, 1, 2)"):
            code, out = describe(text)
            assert code == INVALID_ARGUMENT and name in out and "argument" in out, (text, out)
    for text in ("substring(s)", "substring(s, 1, 2, 3)", "substr()", "substr(s)"):
        code, out = describe(text)
        assert code == INVALID_ARGUMENT and "argument" in out, (text, out)
    assert describe("upper(nope, nope)")[0] == INVALID_ARGUMENT     # the count is static: before any lookup


def test_substring_position_and_length():
    for text in ("substring(s from id)", "substring(s from 1 for id)", "substring(s, 1 + 1)", "substring(s, 1.5)", "substring(s, '1')", "substring(s, 3000000000)",
                 "substr(s, 1, 3000000000)", "substring(s, length(s))"):
        assert describe(text)[0] == NOT_SUPPORTED, text
    for text in ("substring(s from 1 for -1)", "substr(s, -5, -2)", "substring('abc' from 1 for -1)"):
        assert describe(text)[0] == INVALID_ARGUMENT, text
    for text in ("substring(s from (1) for ((2)))", "substring(s, -2147483648, 2147483647)", "substring(s from 2147483647 for 2147483647)", "substring(s, 0, 0)"):
        assert describe(text)[0] == 0, text


def test_unknown_names_answer_as_before():
    for name in ("abs", "foo", "concat", "replace", "position", "strpos", "initcap", "reverse", "lpad", "rpad", "Upper2"):
        want = describe(A.UnsupportedExpr(f"Function({name})"))
        assert want[0] != 0 and describe(f"{name}(s)") == want and describe(f"{name}(s, 1)") == want, name
    assert describe("trim(both 'x' from s)") == describe(A.UnsupportedExpr("Function(trim)"))
    assert describe("sum(id) over (order by id)") == describe(A.UnsupportedExpr("Function(sum)"))
    assert describe("count(*)") == describe(A.UnsupportedExpr("Function(count)"))


def test_concat_typing():
    for text, found in (("s || id", "Int32"), ("id || s", "Int32"), ("s || 1", "Int32"), ("b || s", "Boolean"), ("s || length(s)", "Int32"), ("1 || 2", "Int32")):
        code, out = describe(text)
        assert code == INVALID_ARGUMENT and "||" in out and found in out, (text, out)
    for text, head in (("s || t", "result Utf8 scalar=0 len1=0"), ("s || 'x'", "result Utf8 scalar=0 len1=0"), ("'x' || s", "result Utf8 scalar=0 len1=0"),
                       ("'x' || 'y'", "result Utf8 scalar=1 len1=1"), ("s || 'x' || t", "result Utf8 scalar=0 len1=0"), ("(s || 'x') = t", "result Boolean scalar=0 len1=0"),
                       ("s || 'x' like '%ax'", "result Boolean scalar=0 len1=0"), ("length(s || t) > 3", "result Boolean scalar=0 len1=0"),
                       ("length('abc') > 2", "result Boolean scalar=1 len1=1")):
        code, out = describe(text)
        assert code == 0 and out.splitlines()[0] == head, (text, out)
    nine = " || ".join(["s"] * (MAX_PARTS + 1))
    code, out = describe(nine)
    assert code == 0 and out.splitlines()[0] == "result Utf8 scalar=0 len1=0", out
    assert folded(" || ".join(f"'{c}'" for c in "abcdefghij")) == ("Utf8", "abcdefghij")     # a 10-part chain of literals
    assert folded("'a' || upper('b') || substring('xyz' from 2)") == ("Utf8", "aByz")


def strfn_lines(sql):
    """the `strfn ...` lines of a plan description: one per string function of the tree, operands first"""
    code, out = describe(sql)
    assert code == 0, (sql, out)
    lines = out.splitlines()
    assert lines[1].startswith("split "), (sql, out)
    assert all(ln.startswith("strfn ") for ln in lines[2:]), (sql, out)
    return [ln[len("strfn "):] for ln in lines[2:]]


def test_concat_chains_are_flattened_into_one_operation():
    """a chain of up to STRFN_MAX_PARTS operands is ONE operation; the next operand nests the full one as its first part"""
    chain = lambda k: " || ".join(["s", "'-'", "t"][i % 3] for i in range(k))
    assert MAX_PARTS == 8
    assert strfn_lines(chain(2)) == ["concat parts=2"] and strfn_lines(chain(3)) == ["concat parts=3"]
    assert strfn_lines(chain(MAX_PARTS)) == [f"concat parts={MAX_PARTS}"]
    assert strfn_lines(chain(MAX_PARTS + 1)) == [f"concat parts={MAX_PARTS}", "concat parts=2"]
    assert strfn_lines(chain(2 * MAX_PARTS - 1)) == [f"concat parts={MAX_PARTS}", f"concat parts={MAX_PARTS}"]
    assert strfn_lines(chain(2 * MAX_PARTS)) == [f"concat parts={MAX_PARTS}", f"concat parts={MAX_PARTS}", "concat parts=2"]
    # parentheses on the left side are a chain all the same; a chain on the right side is an operand of its own
    assert strfn_lines("(s || t) || s") == ["concat parts=3"] and strfn_lines("s || (t || s)") == ["concat parts=2", "concat parts=2"]
    # literals next to each other fold before they join; a function among the parts is its own line, in front
    assert strfn_lines("'a' || 'b' || s") == ["concat parts=2"] and strfn_lines("s || 'a' || 'b'") == ["concat parts=3"]
    assert strfn_lines("s || upper(t) || s") == ["upper", "concat parts=3"]
    assert strfn_lines("length(s || '-' || t) > 3") == ["concat parts=3", "length"]
    assert strfn_lines("upper(s) = 'AB'") == ["upper"] and strfn_lines("trim(s)") == ["trim"] and strfn_lines("octet_length(s) > 1") == ["octet_length"]
    assert strfn_lines("substring(s from 2 for 3)") == ["substring from=2 for=3"] and strfn_lines("substr(s, -3)") == ["substring from=-3"]
    assert strfn_lines("ltrim(rtrim(lower(s)))") == ["lower", "rtrim", "ltrim"]
    # the descriptions of expressions without a string function are what they were
    code, out = describe("s like 'a%'")
    assert code == 0 and out == "result Boolean scalar=0 len1=0\nsplit LIKE runs as its own kernel\n"


def test_literal_calls_fold_to_the_reference_value():
    n = 0
    for s in R.CORNERS + R.random_strings(60, 7):
        if "\n" in s:
            continue
        b, q = s.encode(), R.sql_quote(s)
        for name, f in R.UNARY.items():
            want = f(b)
            assert folded(f"{name}({q})") == (("Int32", want) if isinstance(want, int) else ("Utf8", want.decode())), (name, s)
            n += 1
        for p, cnt in R.WINDOWS:
            want = R.substring(b, p, cnt).decode()
            assert folded(R.substring_sql(q, p, cnt)) == ("Utf8", want), (s, p, cnt)
            assert folded(R.substring_sql(q, p, cnt, name="substr")) == ("Utf8", want), (s, p, cnt)
            n += 2
        assert folded(f"{q} || '-' || {q}") == ("Utf8", s + "-" + s)
    assert n > 5000
    assert folded("length(upper('héllo') || '日本')") == ("Int32", 7) and folded("octet_length('日本')") == ("Int32", 6)
    assert folded("upper('abc') = 'ABC'") == ("Boolean", 1) and folded("substring('héllo' from 2 for 2) like 'é_'") == ("Boolean", 1)


# ---- the per-row rules alone, under the sanitizers ---------------------------------------------------------------------------
def hexed(b: bytes) -> str:
    return b.hex() if b else "-"


def sanitizer_cases():
    rows = as_bytes(R.CORNERS + R.random_strings(150, 3)) + R.INVALID + [b" " * 70, b"a" * 130, b" " * 64 + b"a" + b" " * 64]
    lines = []
    for b in rows:
        for name in ("upper", "lower", "trim", "ltrim", "rtrim"):
            lines.append(f"{name} {hexed(b)} 0 0 0 {hexed(R.UNARY[name](b))}")
        lines.append(f"length {hexed(b)} 0 0 0 {R.length(b)}")
        for p, n in R.WINDOWS + [(2147483647, 2147483647), (-2147483648, 2147483647), (-2147483648, None), (1, 2147483647)]:
            lines.append(f"substring {hexed(b)} {p} {0 if n is None else 1} {0 if n is None else n} {hexed(R.substring(b, p, n))}")
    return lines


def test_row_functions_under_host_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler on PATH")
    exe = str(tmp_path / "strfn_main")
    flags = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    src = os.path.join(ROOT, "tests", "strfn_main.cpp")
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
