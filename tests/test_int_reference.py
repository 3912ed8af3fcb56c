"""CPU: the exact integer reference (tests/int_reference.py) against pyarrow.compute's checked kernels, and the oracle
against the reference -- on the range-edge tables the GPU tests (tests/test_gpu_int_edges.py) run.  The table conditions
those tests rely on are asserted here, on the reference alone."""
from math import isqrt

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest

from chapterhouseqe_amd.sqlparse import parse_expr
from oracle import oracle as O

from . import int_reference as R
from .cases import empty_aliases
from .helpers import arrays_identical

PA = {"i8": pa.int8(), "i16": pa.int16(), "i32": pa.int32(), "i64": pa.int64(), "u8": pa.uint8(), "u16": pa.uint16(), "u32": pa.uint32(), "u64": pa.uint64()}
TYPE_OPS = [(t, op) for t in R.TYPES for op in R.OPS]
IDS = [f"{t}{op}" for t, op in TYPE_OPS]


def int_array(values, typ):
    return pa.array(np.array(values, dtype=R.TYPES[typ].dtype), PA[typ])


# ---------------------------------------------------------------------------------------------- table conditions
@pytest.mark.parametrize("typ", list(R.TYPES))
def test_specials_contain_the_minimum_set(typ):
    T = R.TYPES[typ]
    lo, hi, w = T.lo, T.hi, T.width
    sp = R.specials(typ)
    want = [lo, lo + 1, lo + 2, hi - 2, hi - 1, hi, 0, 1, 2, 3, 7, 2**(w - 2) - 1, 2**(w - 2), 2**(w - 2) + 1, hi // 2, hi // 2 + 1, lo // 2, lo // 2 + 1, hi // 3]
    mags = [isqrt(hi) - 1, isqrt(hi), isqrt(hi) + 1, 2**(w // 2) - 1, 2**(w // 2), 2**(w // 2) + 1]
    want += mags
    if T.signed:
        want += [-1, -2, -3, -7, lo // 2 - 1] + [-m for m in mags]
    else:
        want += [2**(w - 1) - 1, 2**(w - 1), 2**(w - 1) + 1]
    assert set(want) <= set(sp) and set(R.minimum_specials(typ)) <= set(sp)
    assert len(set(sp)) == len(sp) and all(lo <= v <= hi for v in sp)
    assert isqrt(hi) ** 2 <= hi < (isqrt(hi) + 1) ** 2
    assert len(R.minimum_specials(typ)) == (34 if T.signed else 19)
    assert len(R.pair_table(typ)) == len(sp) ** 2 == len(set(R.pair_table(typ)))
    if w == 64:      # a zero low word: what a conversion to Boolean that looks at one word gets wrong
        assert 2**32 in sp and (not T.signed or -2**32 in sp)


@pytest.mark.parametrize("typ", list(R.TYPES))
def test_failing_pairs_of_the_minimum_set(typ):
    """the counts of the issue this suite answers, on the cross product of the minimum set"""
    T = R.TYPES[typ]
    sp = R.minimum_specials(typ)
    count = lambda op, what: sum(R.tag(R.arith(op, a, b, typ)) == what for a in sp for b in sp)
    if T.signed:
        assert (count("+", R.OVERFLOW), count("-", R.OVERFLOW)) == (177, 177)
        assert [(count(op, R.OVERFLOW), count(op, R.DIV_ZERO)) for op in "/%"] == [(1, 34), (1, 34)]
        assert 700 <= count("*", R.OVERFLOW) <= 770
    else:
        assert [count(op, R.OVERFLOW) for op in "+-*"] == [99, 171, 226]
        assert [(count(op, R.OVERFLOW), count(op, R.DIV_ZERO)) for op in "/%"] == [(0, 19), (0, 19)]


@pytest.mark.parametrize("typ,op", TYPE_OPS, ids=IDS)
def test_every_table_has_ok_pairs_and_every_failure_class(typ, op):
    assert len(R.ok_rows(typ, op)) >= 100
    assert len(R.ok_rows(typ, op)) + len(R.failing_rows(typ, op)) == len(R.pair_table(typ)) <= 1500
    members = R.class_members(typ, op)
    for c in R.required_classes(op, typ):
        assert members.get(c), f"no pair of class {c}"
    for c, rows in members.items():
        want = R.DIV_ZERO if c.startswith("zero") else R.OVERFLOW
        assert all(R.pair_results(typ, op)[i] is want for i in rows) or c == "other"
    T = R.TYPES[typ]
    if op in "/%":
        assert sum(r is R.DIV_ZERO for r in R.pair_results(typ, op)) == len(R.specials(typ))
        assert sum(r is R.OVERFLOW for r in R.pair_results(typ, op)) == (1 if T.signed else 0)
    if typ == "u32" and op == "*":
        assert all(a * b > 2**63 for a, b in (R.pair_table(typ)[i] for i in members["above_2^63"]))
        assert any(2**32 <= a * b <= 2**63 for a, b in R.pair_table(typ))      # ... and the plain kind of overflow next to it


def test_pow2_and_word_tables():
    xs, lits = R.pow2_table()
    assert set(R.specials("i32")) <= set(xs) and len(xs) == len(R.specials("i32")) + 500
    assert lits[:31] == tuple(2**k for k in range(31)) and set(lits[31:]) == {3, 2**30 - 1, 2**30 + 1, 2147483647}
    seeded = xs[len(R.specials("i32")):]
    assert min(seeded) < -2**31 + 2**24 and max(seeded) > 2**31 - 2**24 and sum(v < 0 for v in seeded) == 250
    assert all(sum(-2**31 + q * 2**29 <= v < -2**31 + (q + 1) * 2**29 for v in seeded) >= 50 for q in range(8))
    for t in ("i8", "i16"):
        x, _ = R.pow2_table(t)
        assert set(R.specials(t)) <= set(x) and (t != "i8" or sorted(x) == list(range(-128, 128)))
    # the rounding cases a shift without the bias term gets wrong
    assert R.arith("/", -1, 2, "i32") == 0 and R.arith("%", -1, 2, "i32") == -1
    assert R.arith("/", -2**31, 2**30, "i32") == -2 and R.arith("/", -2**31 + 1, 2**30, "i32") == -1 and R.arith("%", -2**31 + 1, 2**30, "i32") == -(2**30 - 1)
    for t in ("i64", "u64"):
        v = R.word_values(t)
        assert len(set(v)) == 20 and all(R.TYPES[t].lo <= x <= R.TYPES[t].hi for x in v)
        assert any(a != b and (a ^ b) & 0xFFFFFFFF == 0 for a in v for b in v) and any(a != b and (a ^ b) >> 32 == 0 for a in v for b in v)


def test_reference_on_known_values():
    assert R.arith("/", -7, 2, "i32") == -3 and R.arith("%", -7, 2, "i32") == -1 and R.arith("%", 7, -2, "i32") == 1
    assert R.arith("/", -128, -1, "i8") is R.OVERFLOW and R.arith("/", 5, 0, "i8") is R.DIV_ZERO and R.arith("%", -128, 0, "i8") is R.DIV_ZERO
    assert R.MIN_REM_NEG1_OVERFLOWS and R.arith("%", -128, -1, "i8") is R.OVERFLOW and R.arith("%", -127, -1, "i8") == 0
    assert R.arith("*", 65536, 65536, "u32") is R.OVERFLOW and R.arith("*", 65535, 65537, "u32") == 2**32 - 1
    assert R.arith("-", 0, 1, "u64") is R.OVERFLOW and R.arith("+", 2**63, 2**63 - 1, "u64") == 2**64 - 1
    assert R.common_type("u8", "i16") == "i16" and R.common_type("i64", "u32") == "i64" and R.common_type("u16", "i32") == "i32"
    assert R.common_type("u32", "i32") is None and R.common_type("u64", "i64") is None and R.common_type("u16", "i16") is None and R.common_type("i8", "u8") is None
    assert len(R.MIXED_PAIRS) == 18
    assert R.first_error([[1, None, 2], [3, R.DIV_ZERO, R.OVERFLOW]]) == (R.DIV_ZERO, 1) and R.first_error([[1, 2]]) is None
    assert R.first_error([[1, 2, R.OVERFLOW], [R.DIV_ZERO, 1, 1]]) == (R.OVERFLOW, 2)


# ---------------------------------------------------------------------------------------------- against pyarrow
CHECKED = {"+": pc.add_checked, "-": pc.subtract_checked, "*": pc.multiply_checked, "/": pc.divide_checked}


@pytest.mark.parametrize("typ,op", [(t, op) for t, op in TYPE_OPS if op != "%"], ids=[i for i in IDS if "%" not in i])
def test_reference_equals_pyarrow_checked_kernels(typ, op):
    pairs, res = R.pair_table(typ), R.pair_results(typ, op)
    ok = R.ok_rows(typ, op)
    got = CHECKED[op](int_array([pairs[i][0] for i in ok], typ), int_array([pairs[i][1] for i in ok], typ))
    assert arrays_identical(got, int_array([res[i] for i in ok], typ))
    for i in R.failing_rows(typ, op):
        a, b = pairs[i]
        with pytest.raises(pa.ArrowInvalid) as ei:
            CHECKED[op](pa.scalar(a, PA[typ]), pa.scalar(b, PA[typ]))
        assert ("divide by zero" if res[i] is R.DIV_ZERO else "overflow") in str(ei.value), (a, b, ei.value)


@pytest.mark.parametrize("typ", list(R.TYPES))
def test_remainder_through_the_division_identity(typ):
    """pyarrow has no checked remainder: a == (a / b) * b + a % b with the quotient pyarrow confirmed above, |a % b| < |b|,
    and the sign of the dividend"""
    T = R.TYPES[typ]
    for (a, b), r in zip(R.pair_table(typ), R.pair_results(typ, "%")):
        q = R.arith("/", a, b, typ)
        if b == 0:
            assert r is R.DIV_ZERO and q is R.DIV_ZERO
        elif T.signed and a == T.lo and b == -1:
            assert q is R.OVERFLOW and r is (R.OVERFLOW if R.MIN_REM_NEG1_OVERFLOWS else 0)
        else:
            assert a == q * b + r and abs(r) < abs(b) and (r == 0 or (r < 0) == (a < 0)), (a, b, q, r)


# ---------------------------------------------------------------------------------------------- against the oracle
def oracle_value(rec, sql):
    with O.extension_minus():
        return O.compute_value(rec, empty_aliases(rec), parse_expr(sql))[0]


def pair_batch(typ, rows):
    pairs = R.pair_table(typ)
    return pa.RecordBatch.from_arrays([int_array([pairs[i][0] for i in rows], typ), int_array([pairs[i][1] for i in rows], typ)], names=["x", "y"])


@pytest.mark.parametrize("typ,op", TYPE_OPS, ids=IDS)
def test_oracle_arithmetic_equals_reference(typ, op):
    ok, res = R.ok_rows(typ, op), R.pair_results(typ, op)
    got = oracle_value(pair_batch(typ, ok), f"x {op} y")
    assert arrays_identical(got, int_array([res[i] for i in ok], typ)), (typ, op)
    # every failure class: a few ok rows, then one pair of the class -- first, middle and last member
    for c, rows in R.class_members(typ, op).items():
        for i in {rows[0], rows[len(rows) // 2], rows[-1]}:
            with pytest.raises(O.OracleError) as ei:
                oracle_value(pair_batch(typ, ok[:5] + [i]), f"x {op} y")
            assert ei.value.code == R.STATUS[res[i]], (c, R.pair_table(typ)[i], ei.value)


@pytest.mark.parametrize("typ,op", [(t, op) for t, op in TYPE_OPS if op in "/%"], ids=[i for i in IDS if i[-1] in "/%"])
def test_oracle_detects_every_failing_division(typ, op):
    ok, res = R.ok_rows(typ, op), R.pair_results(typ, op)
    for i in R.failing_rows(typ, op):
        with pytest.raises(O.OracleError) as ei:
            oracle_value(pair_batch(typ, ok[:3] + [i]), f"x {op} y")
        assert ei.value.code == R.STATUS[res[i]]


@pytest.mark.parametrize("typ", list(R.TYPES))
def test_oracle_comparisons_and_to_boolean_equal_reference(typ):
    pairs = R.pair_table(typ)
    rec = pair_batch(typ, range(len(pairs)))
    for op in R.CMPS:
        got = oracle_value(rec, f"x {op} y")
        assert got.to_pylist() == [R.compare(op, a, b) for a, b in pairs], op
    assert oracle_value(rec, "x and y").to_pylist() == [R.to_bool(a) and R.to_bool(b) for a, b in pairs]


@pytest.mark.parametrize("l,r", R.MIXED_PAIRS, ids=[f"{l}+{r}" for l, r in R.MIXED_PAIRS])
def test_oracle_widening_equals_reference(l, r):
    ct = R.common_type(l, r)
    pairs = [(a, b) for a in R.specials(l) for b in R.specials(r)]
    for op in "+*":
        ok = [(a, b) for a, b in pairs if R.tag(R.arith(op, a, b, ct)) == "ok"]
        assert len(ok) >= 50
        rec = pa.RecordBatch.from_arrays([int_array([a for a, _ in ok], l), int_array([b for _, b in ok], r)], names=["x", "y"])
        for sql, want in ((f"x {op} y", [R.arith(op, a, b, ct) for a, b in ok]), (f"y {op} x", [R.arith(op, b, a, ct) for a, b in ok])):
            assert arrays_identical(oracle_value(rec, sql), int_array(want, ct)), sql
    rec = pa.RecordBatch.from_arrays([int_array([a for a, _ in pairs], l), int_array([b for _, b in pairs], r)], names=["x", "y"])
    assert oracle_value(rec, "x < y").to_pylist() == [a < b for a, b in pairs]
