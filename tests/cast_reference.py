"""The tests' reference for CAST / TRY_CAST (include/chq.h: chq_expr_cast): the per-row rules on Python
ints, `fractions.Fraction` and `bytes`.  The float conversions are those of tests/float_reference.py, the integer ranges those
of tests/int_reference.py, the Boolean spellings those of tests/typed_reference.py -- used, not re-derived.

A value is: a Boolean as `bool`, an integer as `int`, a float as its BIT PATTERN (`int`), a Utf8 value as `bytes`.
`cast_rows` returns `(values, validity, failed_row_or_None)`: the output of TRY_CAST (a failing row is null) and the first
valid row at which CAST fails."""
import re
from fractions import Fraction

import numpy as np
import pyarrow as pa

from . import float_reference as F
from . import int_reference as I
from .typed_reference import utf8_to_bool

FAIL = "fail"
CAST_ERROR = 24      # chq_status: CHQ_ERR_ARROW_CAST
NOT_SUPPORTED = 30

INTS = tuple(I.TYPES)                       # i8 .. u64
FLOATS = ("f16", "f32", "f64")
FIXED = ("bool",) + INTS + FLOATS
ALL = FIXED + ("utf8",)
# chq_cast_type / sqlast.CastType
CODE = {"bool": 0, "i8": 1, "i16": 2, "i32": 3, "i64": 4, "u8": 5, "u16": 6, "u32": 7, "u64": 8, "f16": 9, "f32": 10, "f64": 11, "utf8": 12}
NAME = {"bool": "Boolean", "i8": "Int8", "i16": "Int16", "i32": "Int32", "i64": "Int64", "u8": "UInt8", "u16": "UInt16", "u32": "UInt32",
        "u64": "UInt64", "f16": "Float16", "f32": "Float32", "f64": "Float64", "utf8": "Utf8"}
ARROW = {"bool": pa.bool_(), "i8": pa.int8(), "i16": pa.int16(), "i32": pa.int32(), "i64": pa.int64(), "u8": pa.uint8(), "u16": pa.uint16(),
         "u32": pa.uint32(), "u64": pa.uint64(), "f16": pa.float16(), "f32": pa.float32(), "f64": pa.float64(), "utf8": pa.utf8()}
# the SQL spelling of a target (Float16 has none: the C ABI only)
SQL = {"bool": "boolean", "i8": "tinyint", "i16": "smallint", "i32": "int", "i64": "bigint", "u8": "tinyint unsigned",
       "u16": "smallint unsigned", "u32": "int unsigned", "u64": "bigint unsigned", "f32": "real", "f64": "double", "utf8": "varchar"}

_INT_TEXT = re.compile(rb"[+-]?[0-9]+")


def supported(src, dst):
    """is (src, dst) a pair the library casts?  (src == dst is the operand itself)"""
    if src == dst:
        return True
    return not ((src in FLOATS and dst == "utf8") or (src == "utf8" and dst in FLOATS))


def can_fail(src, dst):
    if src == dst:
        return False
    if src == "utf8":
        return True
    if dst not in INTS or src == "bool":
        return False
    if src in FLOATS:
        return True
    return I.TYPES[src].lo < I.TYPES[dst].lo or I.TYPES[src].hi > I.TYPES[dst].hi


def cast_value(v, src, dst):
    """one valid value -> the converted value, or FAIL"""
    if src == dst:
        return v
    if dst == "bool":
        if src == "utf8":
            r = utf8_to_bool(v)
            return FAIL if r is None else r
        return F.to_bool(v, src) if src in FLOATS else I.to_bool(v)
    if src == "bool":
        if dst == "utf8":
            return b"true" if v else b"false"
        return F.convert_int(int(v), dst) if dst in FLOATS else int(v)
    if src in INTS:
        if dst == "utf8":
            return str(v).encode()
        if dst in FLOATS:
            return F.convert_int(v, dst)
        return v if I.TYPES[dst].lo <= v <= I.TYPES[dst].hi else FAIL
    if src in FLOATS:
        if dst in FLOATS:
            return F.convert_float(v, src, dst)
        sign, q = F.decode(v, src)
        if q is F.INF or q is F.NAN:
            return FAIL
        t = q.numerator // q.denominator      # q is a magnitude: floor = truncation toward zero
        t = -t if sign else t
        return t if I.TYPES[dst].lo <= t <= I.TYPES[dst].hi else FAIL
    # Utf8 -> integer
    if not _INT_TEXT.fullmatch(v) or (v[:1] == b"-" and not I.TYPES[dst].signed):
        return FAIL
    t = int(v.decode())
    return t if I.TYPES[dst].lo <= t <= I.TYPES[dst].hi else FAIL


def zero(dst):
    return False if dst == "bool" else b"" if dst == "utf8" else 0


def cast_rows(values, validity, src, dst):
    """-> (values, validity, failed_row_or_None); a null or failing row holds zero(dst)"""
    out, valid, failed = [], [], None
    for i, (v, ok) in enumerate(zip(values, validity)):
        r = cast_value(v, src, dst) if ok else None
        if r is FAIL and failed is None:
            failed = i
        good = ok and r is not FAIL
        out.append(r if good else zero(dst))
        valid.append(bool(good))
    return out, valid, failed


# ---- the edge tables -------------------------------------------------------------------------------------------------------
def int_edges(src, dst=None):
    """min, max, 0, +-1 of the source and of every integer target, target min - 1 and max + 1 -- where the source holds them"""
    s = I.TYPES[src]
    vals = {s.lo, s.hi, 0, 1, -1, s.lo + 1, s.hi - 1, 9, 10, 99, 100, -9, -10, -99, -100}
    for t in I.TYPES.values():
        vals |= {t.lo, t.hi, t.lo - 1, t.hi + 1, t.lo + 1, t.hi - 1}
    for f in FLOATS:   # where integer -> float starts to round, and Float16's overflow to infinity
        p = F.FORMATS[f].p
        vals |= {(1 << p) - 1, 1 << p, (1 << p) + 1, (1 << p) + 2, (1 << p) + 3, -(1 << p) - 1, (1 << (p + 1)) + 2, (1 << (p + 1)) + 6}
    vals |= {65504, 65519, 65520, 65521, -65520, 2**63 - 1, 2**64 - 1, 2**53 + 1, 10**18, 10**19, -10**18, 1234567890123456789}
    return sorted(v for v in vals if s.lo <= v <= s.hi)


def float_edges(fmt):
    """the special values of float_reference.py plus, per integer target: +-0, +-0.5, +-0.999.., target max and min as floats
    with the neighbours on both sides, 2^31, 2^63, 2^64, NaN of both signs, +-inf, subnormals (bit patterns)"""
    FM = F.FORMATS[fmt]
    bits = set(F.specials(fmt))
    enc = lambda q: F.encode(q < 0, abs(Fraction(q)), fmt)
    for q in (Fraction(1, 2), Fraction(3, 2), Fraction(5, 2), 1, 2, 127, 128, 129, 255, 256, 32767, 32768, 65535, 65536, 65504, 2**31, 2**32, 2**63, 2**64):
        bits |= {enc(q), enc(-q)}
    below_one = enc(1) - 1                      # 0.999..
    bits |= {below_one, below_one | FM.sign_bit}
    for t in I.TYPES.values():
        for edge in (t.lo, t.hi, t.hi + 1, t.lo - 1):
            b = enc(edge)
            mag = b & ~FM.sign_bit
            for m in (mag - 1, mag, mag + 1):
                if 0 <= m <= FM.inf_bits:
                    bits |= {m | (b & FM.sign_bit)}
            for frac in (Fraction(1, 2), Fraction(-1, 2), Fraction(999, 1000), Fraction(-999, 1000)):
                bits |= {enc(edge + frac)}
    # what rounds at the edge of a NARROWER float: ties and neighbours of its largest finite value and smallest subnormal
    for narrow in FLOATS:
        N = F.FORMATS[narrow]
        if N.p >= FM.p:
            continue
        big = F.decode(N.inf_bits - 1, narrow)[1]
        ulp = Fraction(2) ** (N.emax - N.p + 1)
        tiny = Fraction(2) ** (N.emin - N.p + 1)
        for q in (big, big + ulp / 2, big + ulp / 4, big + ulp, tiny, tiny / 2, tiny * 3 / 2, tiny / 4, tiny * 3 / 4, Fraction(2) ** N.emin,
                  Fraction(2) ** N.emin - tiny / 2, 1 + Fraction(2) ** (1 - N.p) / 2, 1 + Fraction(2) ** (1 - N.p) * 3 / 2):
            b = enc(q)
            bits |= {b, b | FM.sign_bit, b + 1, b - 1}
    return sorted(bits)


def string_edges():
    rows = [b"", b"+", b"-", b"+0", b"-0", b"0", b"007", b"0" * 25 + b"12", b"-" + b"0" * 25 + b"12", b" 1", b"1 ", b"1.0", b"1e3", b"0x10", b"1\x002",
            b"\x00", "١٢٣".encode(), "１２".encode(), b"12a", b"a12", b"--1", b"+-1", b"1+", b"+1", b"-1", b"42", b"99999999999999999999999",
            b"-99999999999999999999999", b"18446744073709551616", b"1" + b"0" * 40]
    for t in I.TYPES.values():
        rows += [str(t.hi).encode(), str(t.hi + 1).encode(), str(t.lo).encode(), str(t.lo - 1).encode(), b"+" + str(t.hi).encode(), b"00" + str(t.hi).encode()]
    seen, out = set(), []
    for r in rows:
        if r not in seen:
            seen.add(r)
            out.append(r)
    return out


def bool_strings():
    return [b"true", b"TRUE", b" t ", b"yes", b"on", b"1", b"false", b"F", b"no", b"off", b"0", b"tr", b"fals", b"", b"maybe", b"2", b"true\x00", b"truee", b"o", b"\xc2\xa0y\xc2\xa0"]


def edges(src):
    if src == "bool":
        return [False, True]
    if src in INTS:
        return int_edges(src)
    if src in FLOATS:
        return float_edges(src)
    return string_edges()


def clean_rows(src, dst):
    """the edge values of `src` that convert to `dst`"""
    pool = bool_strings() if (src, dst) == ("utf8", "bool") else edges(src)
    return [v for v in pool if cast_value(v, src, dst) is not FAIL]


def failing_rows(src, dst):
    pool = bool_strings() if (src, dst) == ("utf8", "bool") else edges(src)
    return [v for v in pool if cast_value(v, src, dst) is FAIL]


# ---- arrays ------------------------------------------------------------------------------------------------------------------
def to_arrow(values, validity, typ):
    """an Arrow array of `typ` holding the reference's values (floats from their bit patterns)"""
    mask = np.array([not v for v in validity], dtype=bool)
    if typ in FLOATS:
        FM = F.FORMATS[typ]
        return pa.array(np.array(values, dtype=FM.utype).view(FM.dtype), ARROW[typ], mask=mask)
    if typ == "utf8":
        return pa.array([v if ok else None for v, ok in zip(values, validity)], pa.binary()).view(pa.utf8())   # (no validation: rows may be invalid UTF-8)
    if typ == "bool":
        return pa.array([bool(v) if ok else None for v, ok in zip(values, validity)], pa.bool_())
    return pa.array(np.array(values, dtype=I.TYPES[typ].dtype), ARROW[typ], mask=mask)


def from_arrow(arr, typ):
    """(values, validity) of an Arrow array in the reference's representation; a null row holds zero(typ)"""
    validity = [v.is_valid for v in arr]
    if typ in FLOATS:
        FM = F.FORMATS[typ]
        raw = np.frombuffer(arr.buffers()[1], dtype=FM.utype, count=len(arr) + arr.offset)[arr.offset:]
        return [int(b) if ok else 0 for b, ok in zip(raw, validity)], validity
    if typ == "utf8":
        return [v.as_py() if ok else b"" for v, ok in zip(arr.view(pa.binary()), validity)], validity
    return [v.as_py() if ok else zero(typ) for v, ok in zip(arr, validity)], validity
