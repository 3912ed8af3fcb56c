"""An exact reference for the float semantics of the path, independent of the oracle and of every FPU: pure Python on
raw bit patterns of binary16 / binary32 / binary64, exact rationals (fractions.Fraction) rounded once, to nearest, ties
to even, with gradual underflow.  numpy appears only for bit views of the tables.

    decode(bits, fmt) -> (sign, value)     value: Fraction | INF | NAN
    encode(sign, magnitude, fmt) -> bits   magnitude: a non-negative Fraction / int
    arith(op, a_bits, b_bits, fmt)         op in "+-*/%"; `%` is C fmod
    convert_int(value, fmt)  convert_float(bits, src, dst)  parse_literal(text)  to_bool(bits, fmt)
    total_order_key(bits, fmt)  compare(op, a_bits, b_bits, fmt)

NaN rules = the ones kernels.hip documents above F32_LOOP (the reference's x86-64 host): an invalid operation on non-NaN
operands yields the NEGATIVE default NaN, a NaN operand propagates -- the first one of the SQL expression, quieted.
Float16 arithmetic is arrow's / `half`'s from_f32(to_f32(a) OP to_f32(b)): two roundings, on purpose.

The second half builds the deterministic tables the CPU and GPU float-edge tests share (fixed seeds; the constructed
pairs are found by searching with the reference itself).  tests/test_float_reference.py asserts their composition.
"""
from __future__ import annotations

import functools
import random
from collections import namedtuple
from fractions import Fraction

import numpy as np

INF = "inf"
NAN = "nan"

Format = namedtuple("Format", "name width p emax emin mbits sign_bit exp_mask man_mask inf_bits quiet_bit default_nan dtype utype")


def _fmt(name, width, p, dtype, utype):
    emax = (1 << (width - p - 1)) - 1
    mb = p - 1
    inf_bits = ((1 << (width - p)) - 1) << mb
    return Format(name, width, p, emax, 1 - emax, mb, 1 << (width - 1), (1 << (width - p)) - 1, (1 << mb) - 1, inf_bits,
                  1 << (mb - 1), (1 << (width - 1)) | inf_bits | (1 << (mb - 1)), dtype, utype)


FORMATS = {"f16": _fmt("f16", 16, 11, np.float16, np.uint16), "f32": _fmt("f32", 32, 24, np.float32, np.uint32),
           "f64": _fmt("f64", 64, 53, np.float64, np.uint64)}
OPS = "+-*/%"
CMPS = ("=", "<>", "<", "<=", ">", ">=")


# ------------------------------------------------------------------------------------------------ decode / encode
@functools.lru_cache(maxsize=1 << 18)
def decode(bits, fmt):
    F = FORMATS[fmt]
    sign = (bits >> (F.width - 1)) & 1
    e = (bits >> F.mbits) & F.exp_mask
    m = bits & F.man_mask
    if e == F.exp_mask:
        return sign, (NAN if m else INF)
    if e == 0:
        k = F.emin - F.mbits
    else:
        m |= 1 << F.mbits
        k = e - F.emax - F.mbits
    return sign, (Fraction(m << k) if k >= 0 else Fraction(m, 1 << -k))


def is_nan(bits, fmt):
    F = FORMATS[fmt]
    return (bits & ~F.sign_bit & ((1 << F.width) - 1)) > F.inf_bits


def _split(q, F):
    """q > 0 -> (e, m, r, den): 2^e <= q < 2^(e+1); q = (m + r / den) * 2^(max(e, emin) - (p - 1)), 0 <= r < den"""
    n, d = q.numerator, q.denominator
    e = n.bit_length() - d.bit_length()
    if (n < (d << e)) if e >= 0 else ((n << -e) < d):
        e -= 1
    qe = max(e, F.emin) - F.mbits
    if qe >= 0:
        d <<= qe
    else:
        n <<= -qe
    m, r = divmod(n, d)
    return e, m, r, d


def encode(sign, q, fmt):
    """round-to-nearest-even of (-1)^sign * q; gradual underflow; overflow -> infinity; the sign of a zero is `sign`"""
    F = FORMATS[fmt]
    s = F.sign_bit if sign else 0
    q = Fraction(q)
    if q < 0:
        raise ValueError("encode takes a magnitude")
    if q == 0:
        return s
    e, m, r, d = _split(q, F)
    if 2 * r > d or (2 * r == d and (m & 1)):
        m += 1
    # m carries the implicit bit of a normal number: adding it to (biased exponent - 1) << mbits also handles the carry
    # into the next binade, and a subnormal (biased exponent 0) that rounds up to the smallest normal
    bits = ((max(e, F.emin) + F.emax - 1) << F.mbits) + m
    return s | min(bits, F.inf_bits)


def rounding_of(q, fmt):
    """how the exact magnitude q > 0 rounds: "exact", "tie-up", "tie-down", "up", "down" (directions on the magnitude)"""
    _, m, r, d = _split(Fraction(q), FORMATS[fmt])
    if r == 0:
        return "exact"
    if 2 * r == d:
        return "tie-up" if m & 1 else "tie-down"
    return "up" if 2 * r > d else "down"


# ------------------------------------------------------------------------------------------------ arithmetic
def _quiet(bits, F):
    return bits | F.quiet_bit


def exact(op, a, b, fmt):
    """the exact signed rational result of finite operands, or None where the operation has none (a non-finite operand,
    division by zero)"""
    sa, va = decode(a, fmt)
    sb, vb = decode(b, fmt)
    if isinstance(va, str) or isinstance(vb, str):
        return None
    x, y = (-va if sa else va), (-vb if sb else vb)
    if op == "+":
        return x + y
    if op == "-":
        return x - y
    if op == "*":
        return x * y
    if y == 0:
        return None
    if op == "/":
        return x / y
    r = va - vb * (va // vb)
    return -r if sa else r


def arith(op, a, b, fmt):
    if fmt == "f16":
        r = arith(op, convert_float(a, "f16", "f32", quiet=False), convert_float(b, "f16", "f32", quiet=False), "f32")
        return convert_float(r, "f32", "f16")
    F = FORMATS[fmt]
    if is_nan(a, fmt):
        return _quiet(a, F)
    if is_nan(b, fmt):
        return _quiet(b, F)
    sa, va = decode(a, fmt)
    sb, vb = decode(b, fmt)
    if op == "-":
        op, sb = "+", sb ^ 1
    if op == "+":
        if va is INF or vb is INF:
            if va is INF and vb is INF and sa != sb:
                return F.default_nan
            return (F.sign_bit if (sa if va is INF else sb) else 0) | F.inf_bits
        x = (-va if sa else va) + (-vb if sb else vb)
        if x == 0:   # x + (-x) = +0; only -0 + -0 = -0
            return F.sign_bit if (sa and sb and va == 0 and vb == 0) else 0
        return encode(x < 0, abs(x), fmt)
    s = sa ^ sb
    if op == "*":
        if va is INF or vb is INF:
            if va == 0 or vb == 0:
                return F.default_nan
            return (F.sign_bit if s else 0) | F.inf_bits
        return encode(s, va * vb, fmt)
    if op == "/":
        if va is INF:
            return F.default_nan if vb is INF else (F.sign_bit if s else 0) | F.inf_bits
        if vb is INF:
            return F.sign_bit if s else 0
        if vb == 0:
            return F.default_nan if va == 0 else (F.sign_bit if s else 0) | F.inf_bits
        return encode(s, va / vb, fmt)
    if op == "%":   # C fmod: exact, the dividend's sign (a zero result included)
        if va is INF or vb == 0:
            return F.default_nan
        if vb is INF:
            return a
        return encode(sa, va - vb * (va // vb), fmt)
    raise ValueError(op)


@functools.lru_cache(maxsize=1 << 18)
def convert_float(bits, src, dst, quiet=True):
    """a float cast.  NaNs keep their sign and the top payload bits that fit; `quiet` sets the quiet bit (arrow-cast and
    `half` do; quiet=False is the interpreter's one-to-one embedding, used where an operation follows that quiets anyway)"""
    S, D = FORMATS[src], FORMATS[dst]
    sign, v = decode(bits, src)
    s = D.sign_bit if sign else 0
    if v is INF:
        return s | D.inf_bits
    if v is NAN:
        m = bits & S.man_mask
        m = m << (D.mbits - S.mbits) if D.mbits >= S.mbits else m >> (S.mbits - D.mbits)
        return s | D.inf_bits | m | (D.quiet_bit if quiet or m == 0 else 0)
    return encode(sign, v, dst)


def convert_int(value, fmt):
    return encode(value < 0, abs(value), fmt)


def parse_literal(text):
    """a decimal SQL literal is a Float32 (Rust's f32::from_str: correctly rounded)"""
    return encode(0, Fraction(text), "f32")


def to_bool(bits, fmt):
    """float -> Boolean under AND / OR: value != 0 (a subnormal and a NaN are true, -0.0 is false)"""
    return (bits & ~FORMATS[fmt].sign_bit) != 0


def total_order_key(bits, fmt):
    """IEEE 754 totalOrder as an integer key: -NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN, NaNs by payload"""
    F = FORMATS[fmt]
    return -(bits & ~F.sign_bit) - 1 if bits & F.sign_bit else bits


def compare(op, a, b, fmt):
    ka, kb = total_order_key(a, fmt), total_order_key(b, fmt)
    return {"=": a == b, "<>": a != b, "<": ka < kb, "<=": ka <= kb, ">": ka > kb, ">=": ka >= kb}[op]


# ------------------------------------------------------------------------------------------------ over arrays
def arith_bits(op, a, b, fmt):
    """elementwise arith over two equally long sequences of bit patterns -> numpy array of the format's unsigned type"""
    return np.array([arith(op, int(x), int(y), fmt) for x, y in zip(a, b)], dtype=FORMATS[fmt].utype)


def compare_bits(op, a, b, fmt):
    return np.array([compare(op, int(x), int(y), fmt) for x, y in zip(a, b)], dtype=bool)


@functools.lru_cache(maxsize=None)
def table_result(name, op, fmt):
    """reference bits of `x op y` over pair_table(fmt) (name "pairs") or the Float16 sweep (name "sweep"); computed once"""
    a, b = pair_table(fmt) if name == "pairs" else f16_sweep()
    r = arith_bits(op, a, b, fmt)
    r.setflags(write=False)
    return r


# ------------------------------------------------------------------------------------------------ the tables
P = 4096
N_CONSTRUCTED = 64


def specials(fmt):
    """26 magnitudes, both signs = 52 bit patterns.  (2.0, a power of two next to 1.5 and 3, gives exact quotients and
    halvings into the subnormal range)"""
    F = FORMATS[fmt]
    enc = lambda q: encode(0, q, fmt)
    one = enc(1)
    mags = [
        0, 1, (1 << (F.mbits - 1)) | 3, F.man_mask,                 # zero; smallest, a middle and the largest subnormal
        1 << F.mbits, (1 << F.mbits) + 1,                           # smallest normal, 1 ulp above
        one - 1, one, one + 1, enc(Fraction(3, 2)), enc(2), enc(3), enc(10),
        enc(Fraction(1, 10)), enc(Fraction(1, 3)),
        enc((1 << F.p) - 1), enc(1 << F.p), enc((1 << F.p) + 2),
        enc(1 << (F.emax // 2)), enc(1 << F.emax), F.inf_bits - 1, F.inf_bits - 2,
        F.inf_bits,
        F.inf_bits | F.quiet_bit | 0x25, F.inf_bits | F.quiet_bit, F.inf_bits | 0x15,   # qNaN + payload, qNaN, sNaN + payload
    ]
    assert len(set(mags)) == 26
    return mags + [m | F.sign_bit for m in mags]


def _rand_finite(rng, F, elo=None, ehi=None):
    """a random finite pattern whose biased exponent lies in [elo, ehi] (0 = subnormal)"""
    e = rng.randint(0 if elo is None else elo, F.exp_mask - 1 if ehi is None else ehi)
    return (rng.getrandbits(1) << (F.width - 1)) | (e << F.mbits) | rng.getrandbits(F.mbits)


def _exponent(q):
    """floor(log2(q)) of a positive rational"""
    n, d = q.numerator, q.denominator
    e = n.bit_length() - d.bit_length()
    return e - 1 if ((n < (d << e)) if e >= 0 else ((n << -e) < d)) else e


def result_class(op, a, b, fmt):
    """what makes the pair interesting for `op`: "tie-up" / "tie-down" (the exact result lies halfway between two
    neighbours, below the overflow threshold), "subnormal" (the result is a non-zero subnormal), "over" (the exact result
    lies strictly between the largest finite value and 2^(emax+1)), or None.
    No quotient of two floats lies in that open interval: v = 2^(emax+1) * b is itself a float (or overflows, and then
    a / b is below the largest finite value), and no float lies in (v * (1 - 2^-p), v).  For `/` the class is therefore the
    nearest thing that exists: "over-fin", a quotient within the last four finite values, and "over-inf", a quotient from
    2^(emax+1) to less than four such steps above it"""
    F = FORMATS[fmt]
    x = exact(op, a, b, fmt)
    if x is None or x == 0:
        return None
    x = abs(x)
    top = decode(F.inf_bits - 1, fmt)[1]
    if op == "/":
        if decode(F.inf_bits - 4, fmt)[1] <= x <= top:
            return "over-fin"
        if (1 << (F.emax + 1)) <= x < (1 << (F.emax + 1)) + 4 * (top - decode(F.inf_bits - 2, fmt)[1]):
            return "over-inf"
    if x > top:
        return "over" if x < (1 << (F.emax + 1)) else None
    how = rounding_of(x, fmt)
    if how.startswith("tie"):
        return how
    r = encode(0, x, fmt)
    return "subnormal" if 0 < r < (1 << F.mbits) else None


def _candidates(op, want, fmt, rng):
    """proposals that often land in class `want` for `op`; every one is checked with result_class before it is kept"""
    F = FORMATS[fmt]
    top = F.inf_bits - 1
    while True:
        if want == "tie":
            if op == "+":     # neighbouring binades: the sum needs one bit more than the format has
                e = rng.randint(2, F.exp_mask - 2)
                s = rng.getrandbits(1) << (F.width - 1)
                yield s | (e << F.mbits) | rng.getrandbits(F.mbits), s | ((e - 1) << F.mbits) | rng.getrandbits(F.mbits) | 1
            elif op == "*":   # a small odd factor: the product is one or two bits too long, half of the time ...1
                k = encode(0, rng.choice([3, 5, 7, 9]) * Fraction(2) ** rng.randint(-3, 3), fmt)
                yield _rand_finite(rng, F, F.emax // 2, F.emax), k | (rng.getrandbits(1) << (F.width - 1))
            else:             # a quotient ties only below the normal range: halve an odd pattern into the subnormals
                k = rng.randint(1, 6)
                a = (rng.randint(1, k) << F.mbits) | (rng.getrandbits(F.mbits) & ~((1 << k) - 1)) | (1 << rng.randint(0, k - 1))
                yield a | (rng.getrandbits(1) << (F.width - 1)), encode(rng.getrandbits(1), 1 << k, fmt)
        elif want == "subnormal":
            if op == "+":
                yield _rand_finite(rng, F, 0, 2), _rand_finite(rng, F, 0, 2)
            elif op == "*":
                a = _rand_finite(rng, F, 1, F.exp_mask - 1)
                eb = F.emax - ((a >> F.mbits) & F.exp_mask) + F.emin - rng.randint(0, F.mbits - 1)   # product in [2^(emin-p+1), 2^emin)
                if 1 <= eb + F.emax <= F.exp_mask - 1:
                    yield a, (rng.getrandbits(1) << (F.width - 1)) | ((eb + F.emax) << F.mbits) | rng.getrandbits(F.mbits)
            else:
                b = _rand_finite(rng, F, 1, F.exp_mask - 1)
                ea = ((b >> F.mbits) & F.exp_mask) - F.emax + F.emin - rng.randint(1, F.mbits - 1)
                if 1 <= ea + F.emax <= F.exp_mask - 1:
                    yield (rng.getrandbits(1) << (F.width - 1)) | ((ea + F.emax) << F.mbits) | rng.getrandbits(F.mbits), b
        else:   # "over": just past the largest finite value, on either side of the overflow threshold
            if op == "+":
                s = rng.getrandbits(1) << (F.width - 1)
                yield s | (top - rng.randint(0, 3)), s | ((F.exp_mask - 1 - F.p + rng.randint(-1, 2)) << F.mbits) | rng.getrandbits(F.mbits)
            else:
                b = _rand_finite(rng, F, F.emax // 2, F.emax + F.emax // 2) & ~F.sign_bit
                vb = decode(b, fmt)[1]
                vt = decode(top, fmt)[1]
                a = encode(0, vt / vb if op == "*" else vt * vb, fmt)
                if a < F.inf_bits - 8:
                    s = rng.getrandbits(1) << (F.width - 1)
                    yield (a + rng.randint(-3, 3)) | s, b | (rng.getrandbits(1) << (F.width - 1))


def _search(op, want, fmt, rng, count=N_CONSTRUCTED):
    out, ups, downs = [], 0, 0
    for a, b in _candidates(op, want, fmt, rng):
        c = result_class(op, a, b, fmt)
        if c is None or not c.startswith(want) or (a, b) in out:
            continue
        if c in ("tie-up", "over-inf", "tie-down", "over-fin"):   # half of them round up / overflow, half do not
            up = c in ("tie-up", "over-inf")
            if (ups if up else downs) >= count // 2:
                continue
            ups, downs = ups + up, downs + (not up)
        out.append((a, b))
        if len(out) == count:
            return out


FMOD_GAP = {"f16": 30, "f32": 1 << 7, "f64": 1 << 10}
"""the exponent gap (in binades) a "large gap" fmod pair exceeds.  binary16 spans 40 binades in all, so no pair of halves
lies 2^6 binades apart: its pairs lie more than 30 apart, which makes every quotient larger than 2^6"""


def fmod_gap(a, b, fmt):
    (_, va), (_, vb) = decode(a, fmt), decode(b, fmt)
    if isinstance(va, str) or isinstance(vb, str) or va == 0 or vb == 0:
        return None
    return _exponent(va) - _exponent(vb)


def _fmod_pairs(fmt, rng):
    F = FORMATS[fmt]
    gap, sub = [], []
    while len(gap) < N_CONSTRUCTED:
        b = _rand_finite(rng, F, 0, max(0, F.exp_mask - 2 - FMOD_GAP[fmt]))
        a = _rand_finite(rng, F, F.exp_mask - 1 - rng.randint(0, 3), F.exp_mask - 1)
        g = fmod_gap(a, b, fmt)
        if g is not None and g > FMOD_GAP[fmt] and (a, b) not in gap:
            gap.append((a, b))
    while len(sub) < N_CONSTRUCTED:
        b = (rng.getrandbits(1) << (F.width - 1)) | rng.randint(1, F.man_mask)
        a = _rand_finite(rng, F)
        if (a, b) not in sub:
            sub.append((a, b))
    return gap, sub


@functools.lru_cache(maxsize=None)
def table_parts(fmt):
    """the named parts of the pair table, in table order: [(name, [(a, b), ...]), ...]"""
    F = FORMATS[fmt]
    rng = random.Random(0xF10A7 + F.width)
    sp = specials(fmt)
    parts = [("specials", [(a, b) for a in sp for b in sp])]
    for op in "+*/":
        for want in ("tie", "subnormal", "over"):
            parts.append((f"{want}{op}", _search(op, want, fmt, rng)))
    gap, sub = _fmod_pairs(fmt, rng)
    parts += [("gap%", gap), ("subdiv%", sub)]
    used = sum(len(p) for _, p in parts)
    parts.append(("random", [(rng.getrandbits(F.width), rng.getrandbits(F.width)) for _ in range(P - used)]))
    return parts


@functools.lru_cache(maxsize=None)
def pair_table(fmt):
    """(a, b): two read-only arrays of P bit patterns"""
    F = FORMATS[fmt]
    pairs = [p for _, part in table_parts(fmt) for p in part]
    assert len(pairs) == P
    a = np.array([p[0] for p in pairs], dtype=F.utype)
    b = np.array([p[1] for p in pairs], dtype=F.utype)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


#                 1.0     0.1     65504   min sub  -0.0    inf     sNaN+payload  3.0
SWEEP_RIGHT = [0x3C00, 0x2E66, 0x7BFF, 0x0001, 0x8000, 0x7C00, 0x7D15, 0x4200]


@functools.lru_cache(maxsize=None)
def f16_sweep():
    """every Float16 pattern as the left operand, the eight right operands in turn"""
    a = np.arange(65536, dtype=np.uint16)
    b = np.array(SWEEP_RIGHT, dtype=np.uint16)[np.arange(65536) % 8]
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


INT_TYPES = {"i8": (np.int8, 8, True), "i16": (np.int16, 16, True), "i32": (np.int32, 32, True), "i64": (np.int64, 64, True),
             "u8": (np.uint8, 8, False), "u16": (np.uint16, 16, False), "u32": (np.uint32, 32, False), "u64": (np.uint64, 64, False)}
INT_TARGET = {"i32": "f32", "u32": "f32", "i64": "f64", "u64": "f64"}


def int_range(typ):
    _, w, signed = INT_TYPES[typ]
    return (-(1 << (w - 1)), (1 << (w - 1)) - 1) if signed else (0, (1 << w) - 1)


@functools.lru_cache(maxsize=None)
def int_table(typ):
    """the integers whose conversion to the target float format rounds (or just does not): python ints, in range of `typ`"""
    lo, hi = int_range(typ)
    if typ not in INT_TARGET:
        return (lo, hi)
    w = INT_TYPES[typ][1]
    p = FORMATS[INT_TARGET[typ]].p
    vals = [0, 1, lo, hi, lo + 1, hi - 1, (1 << p) - 1, (1 << p) + 1, (1 << p) + 2, (1 << p) + 3, (1 << (p + 1)) + 2, (1 << (p + 1)) + 6]
    for k in range(p + 1, w):
        vals += [(1 << k) - 1, (1 << k) + 1]
    vals += [-v for v in vals]
    out = []
    for v in vals:
        if lo <= v <= hi and v not in out:
            out.append(v)
    return tuple(out)


LITERALS = ["16777217.0", "0.1", "1.0e-45", "1.0e-46", "1.4e-45", "3.4028235e38", "3.4028236e38", "1.0e39", "0.0", "1.5"]
# constants with the sign bit set that SQL can express (there is no unary minus): the expression, whether it needs the
# Minus extension, and how the reference builds its bits
SIGNED_CONSTANTS = [
    ("0.0 / 0.0", False, lambda: arith("/", parse_literal("0.0"), parse_literal("0.0"), "f32")),
    ("0.0 - 1.5", True, lambda: arith("-", parse_literal("0.0"), parse_literal("1.5"), "f32")),
    ("0.0 * (0.0 - 1.0)", True, lambda: arith("*", parse_literal("0.0"), arith("-", parse_literal("0.0"), parse_literal("1.0"), "f32"), "f32")),
]
ARITH_LITERALS = ["1.5", "3.0", "0.1", "16777216.0", "1.0e-45", "3.4028235e38"]
