"""CPU: the exact float reference (tests/float_reference.py) against this host's FPU through numpy, and the oracle against
the reference -- on the edge-value tables the GPU tests (tests/test_gpu_float_edges.py) run.  numpy is compared on the rows
whose result is not a NaN (which NaN an FPU hands back is the host's business); the oracle on every row, NaN bits included."""
from fractions import Fraction

import numpy as np
import pyarrow as pa
import pytest

from chapterhouseqe_amd.sqlparse import parse_expr
from oracle import oracle as O

from . import float_reference as R
from .cases import empty_aliases

FMTS = ("f16", "f32", "f64")
PA = {"f16": pa.float16(), "f32": pa.float32(), "f64": pa.float64()}
TABLES = [("pairs", f) for f in FMTS] + [("sweep", "f16")]


def operands(name, fmt):
    return R.pair_table(fmt) if name == "pairs" else R.f16_sweep()


def float_array(bits, fmt):
    return pa.array(np.asarray(bits, dtype=R.FORMATS[fmt].utype).view(R.FORMATS[fmt].dtype), PA[fmt])


def bits_of(arr, fmt):
    assert arr.type == PA[fmt] and arr.null_count == 0
    return arr.to_numpy(zero_copy_only=False).view(R.FORMATS[fmt].utype)


def report(got, want, a, b):
    bad = np.nonzero(got != want)[0]
    return f"{len(bad)} rows differ, first: " + ", ".join(f"a={int(a[i]):#x} b={int(b[i]):#x} got {int(got[i]):#x} want {int(want[i]):#x}" for i in bad[:4])


# ---------------------------------------------------------------------------------------------- table conditions
@pytest.mark.parametrize("fmt", FMTS)
def test_table_composition(fmt):
    F = R.FORMATS[fmt]
    parts = dict(R.table_parts(fmt))
    a, b = R.pair_table(fmt)
    assert len(a) == len(b) == R.P == 4096
    sp = R.specials(fmt)
    assert len(set(sp)) == 52 and len(parts["specials"]) == 52 * 52 == len(set(parts["specials"]))
    top = R.decode(F.inf_bits - 1, fmt)[1]
    for op in "+*/":
        classes = [R.result_class(op, x, y, fmt) for x, y in parts["tie" + op]]
        assert len(set(parts["tie" + op])) >= 64 and classes.count("tie-up") >= 24 and classes.count("tie-down") >= 24
        assert classes.count("tie-up") + classes.count("tie-down") == len(classes)
        sub = [R.arith(op, x, y, fmt) & ~F.sign_bit for x, y in parts["subnormal" + op]]
        assert len(set(parts["subnormal" + op])) >= 64 and all(0 < r < (1 << F.mbits) for r in sub)
        over = [abs(R.exact(op, x, y, fmt)) for x, y in parts["over" + op]]
        assert len(set(parts["over" + op])) >= 64
        if op != "/":
            assert all(top < q < (1 << (F.emax + 1)) for q in over)
        else:   # no quotient lies in that interval (float_reference.result_class): the last finite values and just past 2^(emax+1)
            assert sum(q <= top for q in over) >= 24 and sum(q >= (1 << (F.emax + 1)) for q in over) >= 24
            assert all(R.decode(F.inf_bits - 4, fmt)[1] <= q < (1 << (F.emax + 1)) * (1 + Fraction(1, 1 << (F.p - 3))) for q in over)
    assert len(set(parts["gap%"])) >= 64 and all(R.fmod_gap(x, y, fmt) > R.FMOD_GAP[fmt] for x, y in parts["gap%"])
    assert R.FMOD_GAP["f32"] == 2**7 and R.FMOD_GAP["f64"] == 2**10
    assert len(set(parts["subdiv%"])) >= 64 and all(0 < (y & ~F.sign_bit) < (1 << F.mbits) for _, y in parts["subdiv%"])
    for op in R.OPS:   # NaN results: at most a quarter of the table
        r = R.table_result("pairs", op, fmt)
        assert sum(R.is_nan(int(v), fmt) for v in r) <= R.P // 4, op


def test_sweep_and_integer_tables():
    a, b = R.f16_sweep()
    assert len(a) == 65536 and len(set(a.tolist())) == 65536 and b[:8].tolist() == R.SWEEP_RIGHT and b[8:16].tolist() == R.SWEEP_RIGHT
    # NaN results stay within a quarter of the sweep, except for `%`: two of the eight right operands make every row a NaN
    # (fmod(x, -0.0), the signalling NaN) -- a quarter -- and among the other six so do the NaN and infinite left operands
    nan_or_inf = lambda v: (v & 0x7FFF) >= 0x7C00
    for op in R.OPS:
        nans = sum(R.is_nan(int(v), "f16") for v in R.table_result("sweep", op, "f16"))
        if op == "%":
            assert nans == 65536 // 4 + sum(nan_or_inf(int(x)) for x, y in zip(a, b) if int(y) not in (0x8000, 0x7D15))
        else:
            assert nans <= 65536 // 4, op
    for typ, fmt in R.INT_TARGET.items():
        p, (lo, hi) = R.FORMATS[fmt].p, R.int_range(typ)
        t = R.int_table(typ)
        want = [0, 1, lo, hi, 2**p - 1, 2**p + 1, 2**p + 2, 2**p + 3, 2**(p + 1) + 2]
        want += [v for k in range(p + 1, R.INT_TYPES[typ][1]) for v in (2**k - 1, 2**k + 1) if v <= hi]
        if lo < 0:
            want += [-1, -(2**p + 1), -(2**p + 3)]
        assert set(want) <= set(t) and all(lo <= v <= hi for v in t)
        assert R.convert_int(2**(p + 1) + 2, fmt) == R.convert_int(2**(p + 1), fmt)     # the tie goes to even
        assert R.convert_int(2**p + 3, fmt) == R.convert_int(2**p + 4, fmt)
    assert R.int_table("i8") == (-128, 127) and R.int_table("u16") == (0, 65535)


def test_reference_on_known_values():
    assert R.parse_literal("16777217.0") == 0x4B800000 and R.parse_literal("0.1") == 0x3DCCCCCD
    assert R.parse_literal("1.0e-45") == 1 and R.parse_literal("1.0e-46") == 0 and R.parse_literal("1.4e-45") == 1
    assert R.parse_literal("3.4028235e38") == 0x7F7FFFFF and R.parse_literal("3.4028236e38") == 0x7F800000 and R.parse_literal("1.0e39") == 0x7F800000
    assert [c[2]() for c in R.SIGNED_CONSTANTS] == [0xFFC00000, 0xBFC00000, 0x80000000]
    assert R.arith("+", 0x3C00, 0xBC00, "f16") == 0 and R.arith("+", 0x8000, 0x8000, "f16") == 0x8000
    assert R.arith("%", 0xC600, 0x4200, "f16") == 0x8000                 # fmod(-6, 3) = -0
    assert R.arith("*", 0x7D15, 0x3C00, "f16") == 0x7F15 and R.arith("/", 0, 0x8000, "f16") == 0xFE00
    keys = [R.total_order_key(b, "f32") for b in (0xFFC00000, 0xFF800000, 0x80000001, 0x80000000, 0, 1, 0x7F800000, 0x7FC00000)]
    assert keys == sorted(keys) and len(set(keys)) == 8
    assert R.to_bool(1, "f64") and not R.to_bool(1 << 63, "f64") and R.to_bool(0x7E00, "f16")


# ---------------------------------------------------------------------------------------------- against the hardware
@pytest.mark.parametrize("name,fmt", TABLES)
@pytest.mark.parametrize("op", R.OPS)
def test_reference_equals_numpy_where_the_result_is_not_nan(name, fmt, op):
    F = R.FORMATS[fmt]
    a, b = operands(name, fmt)
    x, y = a.view(F.dtype), b.view(F.dtype)
    if fmt == "f16":
        x, y = x.astype(np.float32), y.astype(np.float32)
    with np.errstate(all="ignore"):
        n = {"+": np.add, "-": np.subtract, "*": np.multiply, "/": np.divide, "%": np.fmod}[op](x, y).astype(F.dtype)
    want = R.table_result(name, op, fmt)
    keep = np.array([not R.is_nan(int(v), fmt) for v in want])
    assert np.array_equal(np.isnan(n), ~keep)
    got = n.view(F.utype)
    assert np.array_equal(got[keep], want[keep]), report(got[keep], want[keep], a[keep], b[keep])


# ---------------------------------------------------------------------------------------------- against the oracle
def pair_batch(name, fmt):
    a, b = operands(name, fmt)
    return pa.RecordBatch.from_arrays([float_array(a, fmt), float_array(b, fmt), pa.array(np.ones(len(a), dtype=bool))], names=["x", "y", "t"])


def oracle_value(rec, sql):
    return O.compute_value(rec, empty_aliases(rec), parse_expr(sql))[0]


@pytest.mark.parametrize("name,fmt", TABLES)
@pytest.mark.parametrize("op", R.OPS)
def test_oracle_arithmetic_equals_reference(name, fmt, op):
    rec = pair_batch(name, fmt)
    a, b = operands(name, fmt)
    with O.extension_minus():
        got = bits_of(oracle_value(rec, f"x {op} y"), fmt)
    want = R.table_result(name, op, fmt)
    assert np.array_equal(got, want), report(got, want, a, b)


@pytest.mark.parametrize("fmt", FMTS)
def test_oracle_comparisons_and_to_boolean_equal_reference(fmt):
    rec = pair_batch("pairs", fmt)
    a, b = R.pair_table(fmt)
    for op in R.CMPS:
        got = np.asarray(oracle_value(rec, f"x {op} y").to_numpy(zero_copy_only=False))
        want = R.compare_bits(op, a, b, fmt)
        assert np.array_equal(got, want), (op, report(got, want, a, b))
    got = np.asarray(oracle_value(rec, "x and t").to_numpy(zero_copy_only=False))
    want = np.array([R.to_bool(int(v), fmt) for v in a])
    assert np.array_equal(got, want), report(got, want, a, a)


@pytest.mark.parametrize("typ", list(R.INT_TARGET))
def test_oracle_integer_conversions_equal_reference(typ):
    fmt = R.INT_TARGET[typ]
    vals = R.int_table(typ)
    rec = pa.RecordBatch.from_arrays([pa.array(np.array(vals, dtype=R.INT_TYPES[typ][0])), pa.array(np.ones(len(vals)))], names=["i", "one64"])
    got = bits_of(oracle_value(rec, "i * 1.0" if fmt == "f32" else "i * one64"), fmt)
    want = np.array([R.convert_int(v, fmt) for v in vals], dtype=R.FORMATS[fmt].utype)
    assert np.array_equal(got, want), report(got, want, np.array(vals, dtype=object), np.array(vals, dtype=object))


def test_oracle_literals_equal_reference():
    rec = pa.RecordBatch.from_arrays([pa.array([1], pa.int32())], names=["i"])
    for text in R.LITERALS:
        arr, scalar = O.compute_value(rec, [[]], parse_expr(text))
        assert scalar and int(bits_of(arr, "f32")[0]) == R.parse_literal(text), text
    with O.extension_minus():
        for sql, _, ref in R.SIGNED_CONSTANTS:
            arr, scalar = O.compute_value(rec, [[]], parse_expr(sql))
            assert scalar and int(bits_of(arr, "f32")[0]) == ref(), sql
