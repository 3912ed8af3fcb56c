"""An exact reference for the checked integer semantics of the path, independent of the oracle and of every ALU: pure
Python on unbounded ints.  numpy appears only as the dtype of the tables.

    arith(op, a, b, typ) -> int | OVERFLOW | DIV_ZERO      op in "+-*/%": arrow-arith's checked kernels as the project encodes them
    compare(op, a, b)   to_bool(a)   common_type(l, r)
    failure_classes(op, a, b, typ)                          which boundary a failing pair sits on
    first_error(nodes)                                      the (status, row) a call must report

Rules (tests/rules.py pins each once; kernels.hip: Interp::arith, run_fast; oracle/chq_oracle.c: INT_ARITH):
  * a zero divisor is DIV_ZERO before anything else;
  * `/` truncates toward zero, `%` takes the sign of the dividend;
  * MIN / -1 is OVERFLOW; MIN % -1 is OVERFLOW while MIN_REM_NEG1_OVERFLOWS holds (the one place that decision lives in the
    tests -- see the comment above `i8_min_div_neg1_overflows` in rules.py), 0 otherwise; x % -1 = 0 away from MIN;
  * every other result is range-checked against the declared type.

The second half builds the deterministic tables the CPU and GPU integer-edge tests share; tests/test_int_reference.py
asserts their composition.
"""
from __future__ import annotations

import functools
import random
from collections import namedtuple
from math import isqrt

import numpy as np

OVERFLOW = "overflow"
DIV_ZERO = "div_zero"
STATUS = {OVERFLOW: 20, DIV_ZERO: 21}      # chq_status: ARROW_ARITHMETIC_OVERFLOW, ARROW_DIVIDE_BY_ZERO
MIN_REM_NEG1_OVERFLOWS = True

IntType = namedtuple("IntType", "name width signed lo hi dtype")


def _typ(name, width, signed, dtype):
    return IntType(name, width, signed, -(1 << (width - 1)) if signed else 0, (1 << (width - 1)) - 1 if signed else (1 << width) - 1, dtype)


TYPES = {"i8": _typ("i8", 8, True, np.int8), "i16": _typ("i16", 16, True, np.int16), "i32": _typ("i32", 32, True, np.int32),
         "i64": _typ("i64", 64, True, np.int64), "u8": _typ("u8", 8, False, np.uint8), "u16": _typ("u16", 16, False, np.uint16),
         "u32": _typ("u32", 32, False, np.uint32), "u64": _typ("u64", 64, False, np.uint64)}
OPS = "+-*/%"
CMPS = ("=", "<>", "<", "<=", ">", ">=")


# ------------------------------------------------------------------------------------------------ semantics
def _trunc_div(a, b):
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def arith(op, a, b, typ):
    T = TYPES[typ]
    assert T.lo <= a <= T.hi and T.lo <= b <= T.hi, (a, b, typ)
    if op == "+":
        w = a + b
    elif op == "-":
        w = a - b
    elif op == "*":
        w = a * b
    else:
        if b == 0:
            return DIV_ZERO
        if op == "/":
            w = _trunc_div(a, b)
        elif T.signed and a == T.lo and b == -1:
            return OVERFLOW if MIN_REM_NEG1_OVERFLOWS else 0
        else:
            w = a - b * _trunc_div(a, b)
    return w if T.lo <= w <= T.hi else OVERFLOW


def compare(op, a, b):
    return {"=": a == b, "<>": a != b, "<": a < b, "<=": a <= b, ">": a > b, ">=": a >= b}[op]


def to_bool(a):
    """integer -> Boolean under AND / OR: value != 0"""
    return a != 0


_WIDEN = {("i8", "i16"): "i16", ("i8", "i32"): "i32", ("i16", "i32"): "i32", ("i8", "i64"): "i64", ("i16", "i64"): "i64", ("i32", "i64"): "i64",
          ("u8", "u16"): "u16", ("u8", "u32"): "u32", ("u16", "u32"): "u32", ("u8", "u64"): "u64", ("u16", "u64"): "u64", ("u32", "u64"): "u64",
          ("u8", "i16"): "i16", ("u8", "i32"): "i32", ("u16", "i32"): "i32", ("u8", "i64"): "i64", ("u16", "i64"): "i64", ("u32", "i64"): "i64"}
MIXED_PAIRS = tuple(_WIDEN)


def common_type(l, r):
    """the integer rows of plan.cpp: common_type (get_common_type of the reference); None = a coercion miss"""
    if l == r:
        return l
    return _WIDEN.get((l, r)) or _WIDEN.get((r, l))


def failure_classes(op, a, b, typ):
    """the boundaries a failing pair sits on, as a tuple of tags (empty for an `ok` pair; ("other",) for a failing pair on
    none of them)"""
    T = TYPES[typ]
    r = arith(op, a, b, typ)
    if r is DIV_ZERO:
        tags = [f"zero_{n}" for n, v in (("lo", T.lo), ("0", 0), ("hi", T.hi)) if a == v]
        return tuple(tags) or ("other",)
    if r is not OVERFLOW:
        return ()
    if op == "/":
        return ("min_div_neg1",)
    if op == "%":
        return ("min_rem_neg1",)
    w = {"+": a + b, "-": a - b, "*": a * b}[op]
    tags = []
    if w == T.hi + 1:
        tags.append("hi+1")
    if w == T.lo - 1:
        tags.append("lo-1")
    far = {"+": [(T.lo, T.lo), (T.hi, T.hi)], "-": [(T.lo, T.hi), (T.hi, T.lo)], "*": [(T.lo, T.lo), (T.hi, T.hi), (T.lo, T.hi), (T.hi, T.lo)]}[op]
    if (a, b) in far:
        tags.append("farthest")
    if typ == "u32" and op == "*" and w > (1 << 63):
        tags.append("above_2^63")
    if not T.signed and op == "-" and w < 0:
        tags.append("negative")
    return tuple(tags) or ("other",)


def required_classes(op, typ):
    """the failure classes that exist for (typ, op) at all"""
    T = TYPES[typ]
    if op in "/%":
        z = ["zero_lo", "zero_0", "zero_hi"]
        return z + ([{"/": "min_div_neg1", "%": "min_rem_neg1"}[op]] if T.signed and (op == "/" or MIN_REM_NEG1_OVERFLOWS) else [])
    if op == "+":
        return ["hi+1", "farthest"] + (["lo-1"] if T.signed else [])
    if op == "-":
        return ["hi+1", "lo-1", "farthest"] if T.signed else ["lo-1", "negative", "farthest"]
    return ["hi+1", "farthest"] + (["lo-1"] if T.signed else []) + (["above_2^63"] if typ == "u32" else [])


def first_error(nodes):
    """nodes: the per-row results of every arithmetic node in the reference's evaluation order (None = a null slot, which is
    not evaluated).  arrow stops at the first node that fails, at its first failing element -> (status, row) or None"""
    for rows in nodes:
        for i, r in enumerate(rows):
            if r is OVERFLOW or r is DIV_ZERO:
                return r, i
    return None


# ------------------------------------------------------------------------------------------------ the tables
def minimum_specials(typ):
    """the values the tables must contain (the issue's list), in range of `typ`"""
    T = TYPES[typ]
    lo, hi, w = T.lo, T.hi, T.width
    r, h, q = isqrt(hi), 1 << (w // 2), 1 << (w - 2)
    vals = [lo, lo + 1, lo + 2, hi - 2, hi - 1, hi, 0, 1, -1, 2, -2, 3, -3, 7, -7]
    for v in (r - 1, r, r + 1, h - 1, h, h + 1):     # the multiplication boundary; 2^(w/2): a zero low word for 64-bit types
        vals += [v, -v]
    vals += [q - 1, q, q + 1, hi // 2, hi // 2 + 1, lo // 2, lo // 2 - 1, lo // 2 + 1, hi // 3]
    if not T.signed:                                 # what a signed compare or a sign extension gets wrong
        vals += [(1 << (w - 1)) - 1, 1 << (w - 1), (1 << (w - 1)) + 1]
    out = []
    for v in vals:
        if lo <= v <= hi and v not in out:
            out.append(v)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def specials(typ):
    """minimum_specials plus, for signed types, +-(hi // 3 + 1): 3 * -(hi // 3 + 1) = lo - 1 is the only product of two
    table values that lands one below the range (2^(w-1) + 1 is divisible by 3 for every width here)"""
    T = TYPES[typ]
    out = list(minimum_specials(typ))
    if T.signed:
        for v in (T.hi // 3 + 1, -(T.hi // 3 + 1)):
            if v not in out:
                out.append(v)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def pair_table(typ):
    """the cross product of the specials: ((a, b), ...)"""
    sp = specials(typ)
    return tuple((a, b) for a in sp for b in sp)


@functools.lru_cache(maxsize=None)
def pair_results(typ, op):
    """arith over pair_table(typ), computed once: a tuple of values / OVERFLOW / DIV_ZERO"""
    return tuple(arith(op, a, b, typ) for a, b in pair_table(typ))


def tag(r):
    return r if r is OVERFLOW or r is DIV_ZERO else "ok"


def ok_rows(typ, op):
    return [i for i, r in enumerate(pair_results(typ, op)) if tag(r) == "ok"]


def failing_rows(typ, op):
    return [i for i, r in enumerate(pair_results(typ, op)) if tag(r) != "ok"]


@functools.lru_cache(maxsize=None)
def class_members(typ, op):
    """failure class -> rows of pair_table(typ)"""
    out = {}
    for i in failing_rows(typ, op):
        for c in failure_classes(op, *pair_table(typ)[i], typ):
            out.setdefault(c, []).append(i)
    return out


POW2_LITERALS = tuple(1 << k for k in range(31))
POW2_NEIGHBOURS = (3, (1 << 30) - 1, (1 << 30) + 1, 2147483647)      # must NOT take the shift-and-mask shortcut
N_POW2_SEEDED = 500


@functools.lru_cache(maxsize=None)
def pow2_table(typ="i32"):
    """(dividends, literals): every special of `typ` plus 500 seeded values spread over its whole range (every value of an
    8-bit type), each to be divided by every literal 2^k, k = 0..30, and by the four neighbour literals"""
    T = TYPES[typ]
    xs = list(specials(typ))
    if T.width == 8:
        xs += [v for v in range(T.lo, T.hi + 1) if v not in xs]
    else:
        rng = random.Random(0x1D17 + T.width)
        step = (T.hi - T.lo + 1) // N_POW2_SEEDED
        xs += [T.lo + k * step + rng.randrange(step) for k in range(N_POW2_SEEDED)]
    return tuple(xs), POW2_LITERALS + POW2_NEIGHBOURS


@functools.lru_cache(maxsize=None)
def word_values(typ):
    """64-bit values made of every combination of four low and five high words: their cross product holds the pairs that
    differ only in the high word and only in the low word"""
    T = TYPES[typ]
    assert T.width == 64
    vals = [(h << 32) | l for h in (0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF) for l in (0, 1, 0x80000000, 0xFFFFFFFF)]
    return tuple(v - (1 << 64) if T.signed and v >> 63 else v for v in vals)


LITERAL_CONSTANTS = (1, 2, 3, 7, 46340, 46341, 1073741824, 2147483647)      # arithmetic against an Int32 column, both orders
CMP_LITERALS = (("0", 0), ("1", 1), ("2147483646", 2147483646), ("2147483647", 2147483647), ("(0 - 1)", -1), ("(0 - 2147483647)", -2147483647))
