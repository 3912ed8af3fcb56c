"""The tests' reference for CASE, COALESCE, NULLIF, BETWEEN and IN lists on Python lists (None = null).  Pinned by
tests/test_case_host.py to sqlite3 and pyarrow.compute; the GPU tests compare the library with it row by row.

A column is a list.  A computed operand of the lazy-error rule is a callable `row -> value` that may raise DivideByZero or
Overflow; `lazy_case` evaluates it on exactly the rows the rule says."""
from __future__ import annotations

import numpy as np

INTS = {"Int8": (-2**7, 2**7 - 1), "Int16": (-2**15, 2**15 - 1), "Int32": (-2**31, 2**31 - 1), "Int64": (-2**63, 2**63 - 1),
        "UInt8": (0, 2**8 - 1), "UInt16": (0, 2**16 - 1), "UInt32": (0, 2**32 - 1), "UInt64": (0, 2**64 - 1)}
FLOATS = ("Float16", "Float32", "Float64")


class DivideByZero(Exception):
    status = 21      # CHQ_ERR_ARROW_DIVIDE_BY_ZERO


class Overflow(Exception):
    status = 20      # CHQ_ERR_ARROW_ARITHMETIC_OVERFLOW


class NoCommonType(Exception):
    status = 9       # CHQ_ERR_UNSUPPORTED_TYPE_COERSION


# ---- result typing: the coercion table of the binary operators -------------------------------------------------------------
def common_type(a: str, b: str) -> str:
    """the type two operands meet in, or NoCommonType.  Utf8 and Boolean go with themselves only; so does every other name
    (a temporal or decimal type, spelled with its parameters: 'Date32', 'Timestamp(s)', 'Decimal128(30,2)')."""
    if a == b:
        return a
    pair = {a, b}
    if a in INTS and b in INTS:
        sa, sb = a.startswith("Int"), b.startswith("Int")
        wa, wb = int(a.lstrip("UInt")), int(b.lstrip("UInt"))
        if sa == sb:
            return a if wa > wb else b
        s, u = (a, b) if sa else (b, a)       # signed with unsigned: the signed type, when it is the wider one
        ws, wu = (wa, wb) if sa else (wb, wa)
        if ws > wu:
            return s
        raise NoCommonType(f"{a} and {b}")
    if a in FLOATS and b in FLOATS:
        return max(a, b, key=FLOATS.index)
    if len(pair & set(FLOATS)) == 1 and len(pair & set(INTS)) == 1:
        f, i = (a, b) if a in FLOATS else (b, a)
        w = int(i.lstrip("UInt"))
        if f == "Float32" and w <= 32:
            return f
        if f == "Float64":
            return f
    raise NoCommonType(f"{a} and {b}")


def result_type(types) -> str:
    """common_type folded left to right"""
    t = types[0]
    for u in types[1:]:
        t = common_type(t, u)
    return t


def cast(v, frm: str, to: str):
    """one value through the widening cast the typing inserts (never fails)"""
    if v is None or frm == to:
        return v
    if to == "Float32":
        return float(np.float32(v))
    if to == "Float64":
        return float(v) if frm != "Float32" else float(np.float32(v))
    assert to in INTS and INTS[to][0] <= v <= INTS[to][1], (v, frm, to)
    return int(v)


# ---- the per-row rule ------------------------------------------------------------------------------------------------------
def choose(conds_row):
    """index of the first condition that is true (None and False are not), or len(conds_row)"""
    for k, c in enumerate(conds_row):
        if c is True:
            return k
    return len(conds_row)


def case_when(conds, results, else_=None):
    """conds[k], results[k], else_: columns (lists) of one length; else_ None = no ELSE"""
    n = len(conds[0])
    out = []
    for i in range(n):
        k = choose([c[i] for c in conds])
        out.append(results[k][i] if k < len(results) else (None if else_ is None else else_[i]))
    return out


def simple_case(x, values, results, else_=None):
    """CASE x WHEN v THEN r: WHEN k is x = v_k, null when either side is"""
    conds = [[None if a is None or b is None else a == b for a, b in zip(x, v)] for v in values]
    return case_when(conds, results, else_)


def coalesce(*cols):
    return case_when([[v is not None for v in c] for c in cols[:-1]], list(cols[:-1]), cols[-1]) if len(cols) > 1 else list(cols[0])


def nullif(a, b):
    eq = [None if x is None or y is None else x == y for x, y in zip(a, b)]
    return case_when([eq], [[None] * len(a)], a)


def broadcast(v, n):
    return [v] * n


# ---- the lazy-error rule ---------------------------------------------------------------------------------------------------
def lazy_case(n, conds, results, else_=None):
    """conds / results / else_: callables row -> value (they may raise).  Order of evaluation, which decides the error that is
    reported: c1 over the rows, .. cn, then r1 .. rn, then the ELSE.  c_k is evaluated on the rows where no earlier condition was
    TRUE (a null one is not), r_k on the rows that take it, the ELSE on the rows where no condition was true."""
    remaining = [True] * n
    take = []
    for c in conds:
        t = [False] * n
        for i in range(n):
            if remaining[i] and c(i) is True:
                t[i] = True
                remaining[i] = False
        take.append(t)
    out = [None] * n
    for t, r in zip(take, results):
        for i in range(n):
            if t[i]:
                out[i] = r(i)
    if else_ is not None:
        for i in range(n):
            if remaining[i]:
                out[i] = else_(i)
    return out


def checked(op, a, b, typ="Int32"):
    """one checked integer operation as the device does it: null in, null out; DivideByZero / Overflow on valid operands"""
    if a is None or b is None:
        return None
    lo, hi = INTS[typ]
    if op in "/%":
        if b == 0:
            raise DivideByZero()
        q = abs(a) // abs(b) * (1 if (a < 0) == (b < 0) else -1)      # truncating, like the hardware
        w = q if op == "/" else a - q * b
        if op == "%" and a == lo and b == -1:
            w = hi + 1
    else:
        w = a + b if op == "+" else a - b if op == "-" else a * b
    if not lo <= w <= hi:
        raise Overflow()
    return w


# ---- BETWEEN and IN: typing-time sugar -------------------------------------------------------------------------------------
def _cmp(op, a, b):
    if a is None or b is None:
        return None
    return {"=": a == b, "<>": a != b, "<": a < b, "<=": a <= b, ">": a > b, ">=": a >= b}[op]


def _and(a, b):      # the library's AND / OR: null when either side is (not Kleene)
    return None if a is None or b is None else a and b


def _or(a, b):
    return None if a is None or b is None else a or b


def between(x, lo, hi, negated=False):
    """x >= lo AND x <= hi; NOT: x < lo OR x > hi"""
    if negated:
        return [_or(_cmp("<", a, l), _cmp(">", a, h)) for a, l, h in zip(x, lo, hi)]
    return [_and(_cmp(">=", a, l), _cmp("<=", a, h)) for a, l, h in zip(x, lo, hi)]


def in_list(x, items, negated=False):
    """x = l1 OR x = l2 ..; NOT: x <> l1 AND x <> l2 ..  (items: literals)"""
    out = []
    for a in x:
        acc = None
        for k, l in enumerate(items):
            one = _cmp("<>" if negated else "=", a, l)
            acc = one if k == 0 else (_and if negated else _or)(acc, one)
        out.append(acc)
    return out


def between_sql(x, lo, hi, negated=False):
    return f"({x} < {lo} or {x} > {hi})" if negated else f"({x} >= {lo} and {x} <= {hi})"


def in_list_sql(x, items, negated=False):
    return "(" + (" and " if negated else " or ").join(f"{x} {'<>' if negated else '='} {l}" for l in items) + ")"
