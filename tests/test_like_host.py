"""CPU: LIKE / NOT LIKE / IS [NOT] NULL without a GPU.  The tests' reference (tests/like_reference.py, a regex restatement)
against sqlite3 and pyarrow.compute.match_like; the grammar; the library's host half (typing, status codes, the compiled
pattern's bound, constant folding with the matcher the device runs) through `chq_plan_describe`; and that matcher alone in
a stand-alone program under the address and undefined-behaviour sanitizers."""
import os
import random
import re
import shutil
import sqlite3
import subprocess

import pyarrow as pa
import pyarrow.compute as pc
import pytest

import chapterhouseqe_amd as chq
from chapterhouseqe_amd import sqlast as A
from chapterhouseqe_amd.sqlparse import SqlParseError, parse_expr, parse_select

from . import like_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIKE_MAX_ELEMS = int(re.search(r"LIKE_MAX_ELEMS\s*=\s*(\d+)", open(os.path.join(ROOT, "chapterhouseqe_amd", "csrc", "like_device.h")).read()).group(1))


def fixed_cases():
    """(string, pattern, escape) of the fixed table"""
    cases = [(s, p, None) for p in R.PATTERNS for s in R.STRINGS]
    return cases + list(R.EXTRA)


def random_cases(n=4000, seed=20261019):
    rng = random.Random(seed)
    alphabet = ["a", "b", "é", "\n", "%", "_", "!"]
    out = []
    for _ in range(n):
        s = "".join(rng.choice(alphabet) for _ in range(rng.randint(0, 8)))
        p = "".join(rng.choice(alphabet) for _ in range(rng.randint(0, 6)))
        esc = rng.choice([None, None, "!"])
        try:
            R.to_regex(p, esc)
        except R.TrailingEscape:
            continue
        out.append((s, p, esc))
    return out


ALL_CASES = fixed_cases() + random_cases()


# ---- the reference against two independent implementations ------------------------------------------------------------
def test_reference_agrees_with_sqlite():
    db = sqlite3.connect(":memory:")
    db.execute("PRAGMA case_sensitive_like=ON")
    assert len(ALL_CASES) > 3000
    for s, p, esc in ALL_CASES:
        if esc is None:
            got = db.execute("select ? like ?", (s, p)).fetchone()[0]
        else:
            got = db.execute("select ? like ? escape ?", (s, p, esc)).fetchone()[0]
        assert bool(got) == R.like(s, p, esc), (s, p, esc)


def test_reference_agrees_with_pyarrow_match_like():
    by_pattern = {}
    for s, p, esc in ALL_CASES:
        ap = R.arrow_pattern(p, esc)
        if ap is not None:
            by_pattern.setdefault((p, esc, ap), []).append(s)
    assert len(by_pattern) > 500
    for (p, esc, ap), strings in by_pattern.items():
        got = pc.match_like(pa.array(strings, pa.utf8()), ap).to_pylist()
        assert got == [R.like(s, p, esc) for s in strings], (p, esc, strings)


def test_reference_corners():
    assert R.like("aaab", "%aab%") and R.like("abab", "%ab%ab%") and R.like("abaab", "%ab%ab%") and not R.like("aba", "%ab%ab%")
    assert R.like("héllo", "h_llo") and not R.like("héllo", "h__llo") and R.like("a\nb", "a_b") and R.like("", "%") and not R.like("", "_")
    assert R.like("a\\b", "a\\b") and not R.like("a%", "a\\%")   # no default escape
    with pytest.raises(R.TrailingEscape):
        R.like("a", "a!", "!")
    arr = pa.array(["ab", None, "b"])
    assert R.like_array(arr, "a%").to_pylist() == [True, None, False] and R.like_array(arr, "a%", negated=True).to_pylist() == [False, None, True]
    assert R.is_null_array(arr).to_pylist() == [False, True, False] and R.is_null_array(arr, True).to_pylist() == [True, False, True]


# ---- grammar ------------------------------------------------------------------------------------------------------------
S, ID = A.ident("s"), A.ident("id")


def test_grammar_forms():
    assert parse_expr("s like 'a%'") == A.Like(S, A.string("a%"), False, None)
    assert parse_expr("s LIKE 'a%'") == A.Like(S, A.string("a%"), False, None)
    assert parse_expr("s not like 'a%'") == A.Like(S, A.string("a%"), True, None)
    assert parse_expr("s like 'a!%' escape '!'") == A.Like(S, A.string("a!%"), False, "!")
    assert parse_expr("s NOT LIKE 'a!%' ESCAPE '!'") == A.Like(S, A.string("a!%"), True, "!")
    assert parse_expr("s like ('a')") == A.Like(S, A.Nested(A.string("a")), False, None)
    assert parse_expr("s like t") == A.Like(S, A.ident("t"), False, None)     # parses; the evaluator refuses the pattern
    assert parse_expr("s is null") == A.IsNull(S, False)
    assert parse_expr("s IS NOT NULL") == A.IsNull(S, True)
    assert parse_expr("t.s is null") == A.IsNull(A.compound("t", "s"), False)
    assert repr(parse_expr("s not like 'a' escape 'x'")) == ("Like(expr=Identifier(ident=Ident(value='s', quote_style=None)), "
                                                          "pattern=ValueExpr(value=SingleQuotedString(value='a')), negated=True, escape_char='x')")
    assert repr(parse_expr("s is not null")) == "IsNull(expr=Identifier(ident=Ident(value='s', quote_style=None)), negated=True)"


def test_grammar_precedence():
    B, Op = A.BinaryOp, A.BinaryOperator
    like = A.Like(S, A.string("a"), False, None)
    gt = B(ID, Op.Gt, A.number("5"))
    assert parse_expr("s like 'a' and id > 5") == B(like, Op.And, gt)
    assert parse_expr("id > 5 or s like 'a'") == B(gt, Op.Or, like)
    assert parse_expr("id > 5 and s like 'a' or s is null") == B(B(gt, Op.And, like), Op.Or, A.IsNull(S, False))
    # LIKE (19) binds looser than the comparisons (20) and `+` (30), tighter than IS (17), AND and OR
    assert parse_expr("s = t like 'a'") == A.Like(B(S, Op.Eq, A.ident("t")), A.string("a"), False, None)
    assert parse_expr("s like 'a' = true") == A.Like(S, B(A.string("a"), Op.Eq, A.boolean(True)), False, None)
    assert parse_expr("id + 1 is null") == A.IsNull(B(ID, Op.Plus, A.number("1")), False)
    assert parse_expr("id = 1 is not null") == A.IsNull(B(ID, Op.Eq, A.number("1")), True)
    assert parse_expr("s like 'a' is null") == A.IsNull(like, False)
    assert parse_expr("s is null and id is not null") == B(A.IsNull(S, False), Op.And, A.IsNull(ID, True))
    assert parse_expr("(s like 'a') or id is null") == B(A.Nested(like), Op.Or, A.IsNull(ID, False))
    # prefix NOT stays what it was
    assert isinstance(parse_expr("not s like 'a'"), A.UnsupportedExpr) and isinstance(parse_expr("not id > 5"), A.UnsupportedExpr)


def test_grammar_words_as_aliases_parse_as_before():
    sel = parse_select("select id like, s is from read_files('x') escape where s like 'a%' escape '!' and id is not null")
    assert sel.projection == (A.ExprWithAlias(ID, A.Ident("like")), A.ExprWithAlias(S, A.Ident("is")))
    assert sel.from_.alias == "escape"
    assert sel.selection == A.BinaryOp(A.Like(S, A.string("a%"), False, "!"), A.BinaryOperator.And, A.IsNull(ID, True))
    sel = parse_select("select id not, s as like, s like 'a' m, id is null n from read_files('x') as is")
    assert sel.projection == (A.ExprWithAlias(ID, A.Ident("not")), A.ExprWithAlias(S, A.Ident("like")),
                              A.ExprWithAlias(A.Like(S, A.string("a"), False, None), A.Ident("m")), A.ExprWithAlias(A.IsNull(ID, False), A.Ident("n")))
    assert sel.from_.alias == "is"
    sel = parse_select("select s like 'a', s not like 'b' escape 'c', id is not null from read_files('x')")
    assert [type(f) for f in sel.projection] == [A.UnnamedExpr] * 3
    assert sel.projection[1].expr == A.Like(S, A.string("b"), True, "c")


@pytest.mark.parametrize("text", ["s like", "s not like", "s not", "s is", "s is not", "s is not 5", "s is 5", "s like 'a' escape",
                                  "s like 'a' escape 'ab'", "s like 'a' escape ''", "s like 'a' escape x", "s like and id > 5", "like 'a'"])
def test_grammar_malformed(text):
    with pytest.raises(SqlParseError):
        parse_expr(text)


# ---- the library's host half ------------------------------------------------------------------------------------------------
SCHEMA = pa.schema([("s", pa.utf8()), ("id", pa.int32()), ("f", pa.float32())])


def describe(sql, schema=SCHEMA, rows=2):
    try:
        return 0, chq.plan_describe(schema, None, parse_expr(sql), rows)
    except chq.ChqError as e:
        return e.code, str(e)


def folded(sql):
    code, text = describe(sql)
    assert code == 0, (sql, text)
    lines = text.splitlines()
    assert lines[0] in ("result Boolean scalar=1 len1=1", "result Boolean scalar=0 len1=1"), (sql, text)   # (AND / OR clear the scalar flag)
    return int(lines[1].split()[1], 16)


def test_literal_like_folds_to_the_reference_value():
    """the host folds with the matcher the device runs: the whole fixed table, plain and negated"""
    n = 0
    for s, p, esc in fixed_cases():
        want = R.like(s, p, esc)
        assert folded(R.like_sql(R.sql_quote(s), p, esc)) == int(want), (s, p, esc)
        assert folded(R.like_sql(R.sql_quote(s), p, esc, negated=True)) == int(not want), (s, p, esc)
        n += 1
    assert n > 350
    assert folded("'abc' like 'a_c'") == 1 and folded("('abc') like ('a_c')") == 1 and folded("'abc' like 'a_c' and 'x' like '_'") == 1


def test_literal_is_null_folds():
    assert folded("1 is null") == 0 and folded("1 is not null") == 1 and folded("'a' is null") == 0 and folded("1 + 2 is not null") == 1
    assert folded("'maybe' and true is null") == 0      # IS (17) binds tighter than AND: 'maybe' and (true is null)
    assert folded("('maybe' and true) is null") == 1    # a spelling arrow-cast does not know is NULL
    assert folded("'abc' like 'a%' is not null") == 1
    assert describe("1 / 0 is null")[0] == 21           # a literal operand's arithmetic error surfaces as before


def test_column_forms_are_split_off_the_device_program():
    for sql in ["s like 'a%'", "s not like '%a'", "s like 'a!%%' escape '!'", "s is null", "id is not null", "id + 1 is null",
                "s like 'a%' and id > 5", "s is null or id = 3", "(s like '%x%') or f < 1.0"]:
        code, text = describe(sql)
        assert code == 0, (sql, text)
        lines = text.splitlines()
        assert lines[0] == "result Boolean scalar=0 len1=0", (sql, text)
        assert lines[1].startswith("split "), (sql, text)


def test_status_codes():
    assert describe("id like 'a'")[0] == 22 and describe("f not like 'a'")[0] == 22 and describe("1 like '1'")[0] == 22
    assert describe("(id > 1) like 'a'")[0] == 22
    assert describe("s like id")[0] == 30 and describe("s like s")[0] == 30 and describe("'a' like 'a' + 1")[0] == 30
    assert describe("s like 'a!' escape '!'")[0] == 22 and describe("'a' like '!' escape '!'")[0] == 22
    assert describe("s like 'a!!' escape '!'")[0] == 0
    assert describe("nope like 'a'")[0] == describe("nope = 'a'")[0] != 0      # the operand's own errors come first
    assert describe("nope is null")[0] == describe("nope = 1")[0]


def test_pattern_bound():
    """LIKE_MAX_ELEMS elements (literal bytes and `_`; `%` and escape characters do not count) fit, one more does not"""
    at = "%" + "a_" * (LIKE_MAX_ELEMS // 2) + "%"
    assert describe(f"s like '{at}'")[0] == 0
    assert describe("s like '" + "!a" * LIKE_MAX_ELEMS + "%%%' escape '!'")[0] == 0
    code, text = describe(f"s like '{at}b'")
    assert code == 30 and str(LIKE_MAX_ELEMS) in text, text
    assert describe("s like '" + "é" * (LIKE_MAX_ELEMS // 2) + "'")[0] == 0     # two bytes each
    assert describe("s like '" + "é" * (LIKE_MAX_ELEMS // 2) + "_'")[0] == 30
    assert folded("'" + "ab" * (LIKE_MAX_ELEMS // 2) + "' like '" + "a_" * (LIKE_MAX_ELEMS // 2) + "'") == 1


IMPORTABLE = [pa.bool_(), pa.int8(), pa.int16(), pa.int32(), pa.int64(), pa.uint8(), pa.uint16(), pa.uint32(), pa.uint64(), pa.float16(),
              pa.float32(), pa.float64(), pa.utf8(), pa.date32(), pa.date64(), pa.time32("s"), pa.time32("ms"), pa.time64("us"), pa.time64("ns"),
              pa.timestamp("s"), pa.timestamp("us", "UTC"), pa.duration("ms"), pa.decimal128(20, 3), pa.binary(4), pa.binary(16)]


@pytest.mark.parametrize("typ", IMPORTABLE, ids=str)
def test_is_null_types_on_every_importable_column_type(typ):
    schema = pa.schema([("x", typ)])
    for sql in ("x is null", "x is not null", "(x) is null"):
        code, text = describe(sql, schema)
        assert code == 0 and text.splitlines()[0] == "result Boolean scalar=0 len1=0", (typ, sql, text)


# ---- the matcher alone, under the sanitizers -------------------------------------------------------------------------------
def hexed(b: bytes) -> str:
    return b.hex() if b else "-"


def test_matcher_under_host_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler on PATH")
    exe = str(tmp_path / "like_matcher")
    flags = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    src = os.path.join(ROOT, "tests", "like_matcher_main.cpp")
    # the runtimes linked statically where the compiler has them that way: the program then needs nothing from its environment
    build = subprocess.run([cxx, *flags, "-static-libasan", "-static-libubsan", src, "-o", exe], capture_output=True, text=True)
    if build.returncode != 0:
        build = subprocess.run([cxx, *flags, src, "-o", exe], capture_output=True, text=True)
    if build.returncode != 0 and re.search(r"asan|ubsan|sanitize", build.stderr, re.I):
        pytest.skip("the compiler has no sanitizer runtime: " + build.stderr.strip().splitlines()[-1])
    assert build.returncode == 0, build.stderr
    lines = []
    for s, p, esc in ALL_CASES:
        lines.append(f"{hexed(s.encode())} {hexed(p.encode())} {-1 if esc is None else ord(esc)} {int(R.like(s, p, esc))}")
    # the statuses of the compiler, and strings of invalid UTF-8 (stray continuation bytes, truncated characters): the
    # matcher may answer anything there but must stay inside the string -- the expected value is what it gives
    lines.append(f"{hexed(b'a')} {hexed(b'a!')} {ord('!')} E")
    lines.append(f"- {hexed(b'!')} {ord('!')} E")
    lines.append(f"{hexed(b'a')} {hexed(b'a' * (LIKE_MAX_ELEMS + 1))} -1 L")
    lines.append(f"{hexed(b'a' * LIKE_MAX_ELEMS)} {hexed(b'a' * LIKE_MAX_ELEMS)} -1 1")
    lines.append(f"{hexed(b'a' * LIKE_MAX_ELEMS)} {hexed(b'%' + b'_' * LIKE_MAX_ELEMS + b'%')} -1 1")
    for raw, pat, want in [(b"\x80", b"_", 0), (b"\x80\x80", b"%_", 0), (b"a\x80", b"%_", 1), (b"\xc3", b"_", 1), (b"\xc3", b"%_", 1),
                           (b"\xe6\x97", b"_%", 1), (b"\x80a", b"%_", 1), (b"\xbf\xbf\xbf", b"%_%_%", 0), (b"a\xbf\xbf", b"_", 1)]:
        lines.append(f"{hexed(raw)} {hexed(pat)} -1 {want}")
    cases = tmp_path / "cases.txt"
    cases.write_text("\n".join(lines) + "\n")
    run = subprocess.run([exe, str(cases)], capture_output=True, text=True)
    if run.returncode != 0 and "runtime does not come first" in run.stderr:
        pytest.skip("this environment preloads a library in front of the sanitizer runtime: " + run.stderr.strip().splitlines()[0])
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith(f"{len(lines)} cases, 0 mismatches"), run.stdout
