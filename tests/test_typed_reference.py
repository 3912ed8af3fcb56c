"""CPU: the reference of tests/typed_reference.py tied down before the GPU tier uses it, and the two host-side copies of
what the typed kernels compute tied to it: oracle/chq_oracle.c (utf8_bool and its white-space table, the raw-value
comparisons of temporal and Decimal128 columns) and csrc/plan.cpp (utf8_to_bool: the folding of Utf8 literals under AND / OR,
through `chq_plan_describe`; the `left == right` arm of the coercion table).

White space.  `WHITE_SPACE` is compared with Python's own table (`str.isspace` minus U+001C..U+001F, which Rust's
`char::is_whitespace` does not take).  The C tables are written as UTF-8 byte patterns, not code points, so they are pinned
by what they do: the oracle casts ONE column holding every Unicode scalar value c as `c 1 c` -- true exactly for the 25
members -- and the host planner folds the same literal for every c below U+3100 (all members lie there) and for every
non-member the word table names.  A code point a C table names that is not a member would be trimmed and show up as true.

Literal folding.  `chq_plan_describe` prints a folded Boolean as its bits, a NULL as 0, so each word is folded twice:
`'<w>' and true` is 1 exactly for a true spelling, `'<w>' or true` (AND / OR are not Kleene: NULL or true = NULL) is 0
exactly for a NULL.  The SQL tokenizer ends a literal at `'` and the C string of the call ends at NUL: of the 1 901 words
of BOOL_WORD_TABLE 69 hold a NUL and none a quote, so 1 832 are folded; the 69 reach the oracle and the device as column
values."""
import numpy as np
import pyarrow as pa
import pytest

import chapterhouseqe_amd as chq
from chapterhouseqe_amd.sqlparse import parse_expr
from oracle import oracle as O

from . import typed_reference as R
from .helpers import arrays_identical

AL2 = [[], []]


# ---------------------------------------------------------------------------------------------- the reference itself
def test_white_space_is_pythons_table_without_the_information_separators():
    python = {c for c in range(0x110000) if chr(c).isspace()}
    assert set(R.WHITE_SPACE) == python - {0x1C, 0x1D, 0x1E, 0x1F} and len(R.WHITE_SPACE) == len(set(R.WHITE_SPACE)) == 25
    assert not set(R.NOT_WS_TABLE + R.NOT_WS_BYTES) & set(R.WHITE_SPACE)


# worked out by hand from arrow-cast 53's cast_utf8_to_boolean, not by the reference
ANCHORS = [(b"true", True), (b"TrUe", True), (b"tru", True), (b"1", True), (b"on", True), (b"YES", True), (b"\xe2\x80\xa8y\xc2\x85", True),
           (b"false", False), (b"fals", False), (b"OF", False), (b"off", False), (b"0", False), (b"\x0bNo\x0c", False),
           (b"", None), (b" ", None), (b"o", None), (b"falsee", None), (b"treu", None), (b"t rue", None), (b"2", None), (b"-1", None),
           (b"\x1ctrue", None), (b"true\x1f", None), (b"\xe2\x80\x8btrue", None), (b"true\xc3\xa0", None), (b"true\xe2\x82\x80", None),
           (b"true\xe2\x82\xa8", None), (b"true\xe1\x82\xa0", None), (b"\x00true", None), (b"ye\xc5\xbf", None), (b"\xc4\xb0", None),
           (b"\xef\xbd\x94\xef\xbd\x92\xef\xbd\x95\xef\xbd\x85", None), (b"\xe2\x84\xaa", None)]


def test_reference_cast_on_hand_worked_rows():
    table = dict(R.BOOL_WORD_TABLE)
    for word, want in ANCHORS:
        assert R.utf8_to_bool(word) is want, word
        assert word in table and table[word] is want, word
    for s in R.TRUE_SPELLINGS + R.FALSE_SPELLINGS:
        for c in R.WHITE_SPACE:
            w = chr(c).encode()
            assert R.utf8_to_bool(w + s.upper() + w + w) is (s in R.TRUE_SPELLINGS)
            assert R.utf8_to_bool(s[:1] + w + s[1:] + b"x") is None
    assert len(R.TRUE_SPELLINGS) == 9 and len(R.FALSE_SPELLINGS) == 10
    # the table holds what the issue asks for: every case mix, every pad length, the lookalikes on both sides
    assert sum(1 for w, _ in R.BOOL_WORD_TABLE if w.lower() == b"false") == 32 and sum(1 for w, _ in R.BOOL_WORD_TABLE if w.lower() == b"true") == 16
    for n in R.PAD_LENGTHS:
        assert table[b" " * n + b"1" + b" " * n] is True and table[b" " * n] is None
    for c in R.NOT_WS_TABLE + R.NOT_WS_BYTES:
        w = chr(c).encode()
        assert table[w + b"true"] is None and table[b"true" + w] is None and table[b"0" + w + b" "] is None


def test_edge_tables_hold_what_they_promise():
    e = set(R.I128_EDGES)
    want = [0, 1, -1, 2**31, -2**31, 2**32 - 1, 1 - 2**32, 2**32, -2**32, 2**63 - 1, 2**63, -2**63, 2**64 - 1, 2**64, -2**64, -2**64 - 1,
            10**38 - 1, 1 - 10**38, 2**127 - 1, -2**127]
    assert all(v in e for v in want) and len(e) == len(R.I128_EDGES)
    pat = {v & R.M128 for v in e}
    for w in range(4):   # pairs that differ in one 32-bit word only: by 1 and by the word's top bit, other words 0 and all-ones
        for others in (0, R.M128 ^ (0xFFFFFFFF << (32 * w))):
            base = others | (5 << (32 * w))
            assert {base, base + (1 << (32 * w)), base ^ (0x80000000 << (32 * w))} <= pat
    assert {-2**31, -2**31 + 1, -2**16, -1, 0, 1, 2**16, 2**31 - 2, 2**31 - 1} == set(R.I32_EDGES)
    assert {-2**63, -2**63 + 1, -2**32, -2**31 - 1, -2**16, -1, 0, 1, 2**16, 2**31 - 1, 2**31, 2**32 - 1, 2**32, 2**63 - 2, 2**63 - 1} <= set(R.I64_EDGES)
    assert len(R.TEMPORAL_TYPES) == 18 and len({t for _, t in R.TEMPORAL_TYPES}) == 18
    for edges in (R.I128_EDGES, R.I64_EDGES, R.I32_EDGES):
        rows = R.pair_batch_rows(edges)
        assert len(rows) % 64 != 0 and set(rows) == set(R.pair_table(edges))
        n = len(edges) ** 2
        assert all(rows[n + i] == rows[(i + 37) % n] for i in range(n))
    # the builders write the raw patterns
    arr = R.decimal128_array(R.I128_EDGES)
    assert R.decimal_patterns(arr) == R.I128_EDGES and R.decimal_patterns(arr.slice(3, 5)) == R.I128_EDGES[3:8]
    assert arr.buffers()[1].to_pybytes()[:16] == bytes(16) and arr.null_count == 0
    assert R.decimal128_array([2**127 - 1, -2**127]).buffers()[1].to_pybytes() == b"\xff" * 15 + b"\x7f" + bytes(15) + b"\x80"
    assert R.cmp("<", -2**127, 2**127 - 1) and R.cmp(">=", 2**64, 2**64 - 1) and not R.cmp("=", 2**32, 0) and R.cmp("<>", -1, 2**64 - 1)


# ---------------------------------------------------------------------------------------------- oracle: Utf8 -> Boolean
def words_batch(words, flag_value):
    return pa.RecordBatch.from_arrays([R.utf8_array(words), pa.array([flag_value] * len(words), pa.bool_())], names=["s", "b"])


def expected_words(words):
    return R.bool_result([R.utf8_to_bool(w) for w in words])


@pytest.mark.parametrize("op,flag", [("and", True), ("or", False)])
def test_oracle_casts_the_word_table(op, flag):
    words = R.BOOL_WORDS
    got, scalar = O.compute_value(words_batch(words, flag), AL2, parse_expr(f"s {op} b"))
    exp = R.bool_result([e for _, e in R.BOOL_WORD_TABLE])
    bad = [i for i in range(len(words)) if got[i].as_py() != exp[i].as_py()]
    assert not scalar and arrays_identical(got, exp), [(words[i], got[i].as_py(), exp[i].as_py()) for i in bad[:5]]


def code_point_words():
    """`c 1 c` for every Unicode scalar value c"""
    cps = [c for c in range(0x110000) if not 0xD800 <= c <= 0xDFFF]
    return cps, [chr(c).encode("utf-8") + b"1" + chr(c).encode("utf-8") for c in cps]


def test_oracle_trims_exactly_the_white_space_code_points():
    cps, words = code_point_words()
    got, _ = O.compute_value(words_batch(words, True), AL2, parse_expr("s and b"))
    ws = set(R.WHITE_SPACE)
    exp = pa.array([True if c in ws else None for c in cps], pa.bool_())
    trimmed = [hex(c) for c, v in zip(cps, got.is_valid().to_pylist()) if v]
    assert arrays_identical(got, exp), trimmed


# ---------------------------------------------------------------------------------------------- plan.cpp: literal folding
SCHEMA = pa.schema([("id", pa.int32())])


def folded(word: bytes):
    """the value plan.cpp folds a Utf8 literal under AND / OR to"""
    lit = "'" + word.decode("utf-8") + "'"
    bits = []
    for sql in (f"{lit} and true", f"{lit} or true"):
        lines = chq.plan_describe(SCHEMA, None, parse_expr(sql)).splitlines()
        assert lines[0] == "result Boolean scalar=0 len1=1", (word, lines)
        bits.append(int(lines[1].split()[1], 16))
    return None if bits[1] == 0 else bool(bits[0])


def test_host_planner_folds_the_word_table():
    carried = [(w, e) for w, e in R.BOOL_WORD_TABLE if b"'" not in w and b"\x00" not in w]
    assert len(R.BOOL_WORD_TABLE) - len(carried) == 69 and not any(b"'" in w for w in R.BOOL_WORDS)
    bad = [(w, folded(w), e) for w, e in carried if folded(w) is not e]
    assert not bad, bad[:5]


def test_host_planner_trims_exactly_the_white_space_code_points():
    ws = set(R.WHITE_SPACE)
    assert max(ws) < 0x3100
    cps = [c for c in range(1, 0x3100) if c != 0x27] + R.NOT_WS_TABLE[:-1] + R.NOT_WS_BYTES + [0xFEFF, 0xFFFD, 0x10000, 0x10FFFF, 0xE0020, 0x1D7CF]
    trimmed = {c for c in cps if folded(chr(c).encode() + b"1" + chr(c).encode()) is True}
    assert trimmed == ws, sorted(hex(c) for c in trimmed ^ ws)


# ---------------------------------------------------------------------------------------------- oracle: comparisons
def oracle_compare(x, y, op):
    rec = pa.RecordBatch.from_arrays([x, y], names=["x", "y"])
    got, scalar = O.compute_value(rec, AL2, parse_expr(f"x {op} y"))
    assert not scalar
    return got


@pytest.mark.parametrize("op", R.CMPS)
def test_oracle_compares_decimal128_edges(op):
    pairs = R.pair_table(R.I128_EDGES)
    got = oracle_compare(R.decimal128_array([a for a, _ in pairs]), R.decimal128_array([b for _, b in pairs]), op)
    exp = pa.array([R.cmp(op, a, b) for a, b in pairs])
    bad = [pairs[i] for i in range(len(pairs)) if got[i].as_py() != exp[i].as_py()]
    assert arrays_identical(got, exp), bad[:5]


@pytest.mark.parametrize("name,typ", R.TEMPORAL_TYPES, ids=[n for n, _ in R.TEMPORAL_TYPES])
def test_oracle_compares_temporal_edges(name, typ):
    pairs = R.pair_table(R.temporal_edges(typ))
    x, y = R.temporal_array([a for a, _ in pairs], typ), R.temporal_array([b for _, b in pairs], typ)
    for op in R.CMPS:
        got = oracle_compare(x, y, op)
        exp = pa.array([R.cmp(op, a, b) for a, b in pairs])
        bad = [pairs[i] for i in range(len(pairs)) if got[i].as_py() != exp[i].as_py()]
        assert arrays_identical(got, exp), (op, bad[:5])


# ---------------------------------------------------------------------------------------------- static rules
def statuses(tx, ty, op):
    """(oracle status, host planner status) of `x op y` over columns of the two types"""
    x = R.decimal_array([1, 2], None, tx) if pa.types.is_decimal(tx) else R.temporal_array([1, 2], tx)
    y = R.decimal_array([1, 3], None, ty) if pa.types.is_decimal(ty) else R.temporal_array([1, 3], ty)
    rec = pa.RecordBatch.from_arrays([x, y], names=["x", "y"])
    e = parse_expr(f"x {op} y")
    try:
        O.compute_value(rec, AL2, e)
        ocode = 0
    except O.OracleError as err:
        ocode = err.code
    try:
        text = chq.plan_describe(rec.schema, AL2, e, 2)
        assert text.splitlines()[0].startswith("result Boolean scalar=0 len1=0"), text
        code = 0
    except chq.ChqError as err:
        code = err.code
    return ocode, code


def test_only_equal_datatypes_compare():
    D = pa.decimal128
    for tx, ty in [(D(38, 0), D(38, 1)), (D(37, 0), D(38, 0)), (pa.timestamp("us"), pa.timestamp("us", tz="UTC"))]:
        for op in R.CMPS:
            assert statuses(tx, ty, op) == (9, 9) and statuses(ty, tx, op) == (9, 9), (tx, ty, op)
    for typ in [t for _, t in R.TEMPORAL_TYPES] + [D(38, 0), D(38, 1), D(37, 0)]:
        for op in R.CMPS:
            assert statuses(typ, typ, op) == (0, 0), (typ, op)
