"""Exact host references of the typed operations (tests only): Decimal128 and temporal comparisons on edge values, and
arrow-cast 53's `cast_utf8_to_boolean` (the Utf8 -> Boolean cast under AND / OR).  Independent of the oracle and of the
library: plain Python integers and bytes, nothing here calls either.  tests/test_typed_reference.py ties the oracle and
the host planner's literal folding to these tables on the CPU tier, tests/test_gpu_typed_edges.py the kernels of
csrc/typed_ops.hip and the routing around them.

Comparisons: arrow-ord compares the native values (i32 / i64 / i128) of two columns of the same DataType; `cmp` is that on
Python ints.  The decimal table holds raw 128-bit patterns -- 2^127 - 1 and -2^127 lie outside every declared precision,
Arrow does not validate them -- so decimal columns are built with `from_buffers` and never read back through `to_pylist`.

Utf8 -> Boolean: `value.to_ascii_lowercase().trim()` matched against the accepted spellings, anything else NULL.  Rust's
`trim` removes the 25 code points of Unicode White_Space (`char::is_whitespace`) and `to_ascii_lowercase` folds A-Z only;
Python's `str.strip` / `str.isspace` also take U+001C..U+001F and `str.lower` folds non-ASCII letters, so none of them is
used: the reference works on bytes.
"""
from __future__ import annotations

import itertools
from typing import List, Optional, Sequence, Tuple

import numpy as np
import pyarrow as pa

CMPS = ("=", "<>", "<", "<=", ">", ">=")


def cmp(op: str, a: int, b: int) -> bool:
    return {"=": a == b, "<>": a != b, "<": a < b, "<=": a <= b, ">": a > b, ">=": a >= b}[op]


# ---- Decimal128 -------------------------------------------------------------------------------------------------------------
M128 = (1 << 128) - 1


def i128(pattern: int) -> int:
    """the signed value of a raw 128-bit pattern"""
    pattern &= M128
    return pattern - (1 << 128) if pattern >> 127 else pattern


def _word_variants() -> List[int]:
    """for each of the four 32-bit words: a base value and three variants that differ from it in that word only -- by 1, by
    0x8000_0000 and by both -- with the other three words zero and with them all-ones"""
    out = []
    for w in range(4):
        hole = M128 ^ (0xFFFFFFFF << (32 * w))
        for others in (0, hole):
            for word in (0x00000005, 0x00000006, 0x80000005, 0x80000006):
                out.append(i128(others | (word << (32 * w))))
    return out


def _unique(values: Sequence[int]) -> List[int]:
    seen, out = set(), []
    for v in values:
        if v not in seen:
            seen.add(v)
            out.append(v)
    return out


I128_EDGES: List[int] = _unique(
    [0, 1, -1, 2**31, -2**31, 2**32 - 1, -(2**32 - 1), 2**32, -2**32, 2**63 - 1, 2**63, -2**63, 2**64 - 1, 2**64, -2**64, -2**64 - 1,
     10**38 - 1, -(10**38 - 1), 2**127 - 1, -2**127] + _word_variants())
assert all(-2**127 <= v < 2**127 for v in I128_EDGES) and 48 <= len(I128_EDGES) <= 60


def validity_buffer(valid) -> Optional[pa.Buffer]:
    return None if valid is None else pa.py_buffer(np.packbits(np.asarray(valid, dtype=bool), bitorder="little").tobytes())


def decimal_array(values: Sequence[int], valid=None, typ: pa.DataType = pa.decimal128(38, 0)) -> pa.Array:
    """raw little-endian two's complement patterns of the type's width, whatever its precision says; `valid`: a Boolean per
    row (a bitmap is then present even when every row is valid)"""
    width = typ.bit_width // 8
    data = b"".join((int(v) & ((1 << (8 * width)) - 1)).to_bytes(width, "little") for v in values)
    nulls = 0 if valid is None else int(len(values) - np.count_nonzero(valid))
    return pa.Array.from_buffers(typ, len(values), [validity_buffer(valid), pa.py_buffer(data)], null_count=nulls)


def decimal128_array(values: Sequence[int], valid=None) -> pa.Array:
    return decimal_array(values, valid, pa.decimal128(38, 0))


def decimal_patterns(arr: pa.Array) -> List[int]:
    """the raw values of a decimal array as signed ints (null slots included), read from its buffer"""
    width = arr.type.bit_width // 8
    raw = arr.buffers()[1].to_pybytes()[arr.offset * width:(arr.offset + len(arr)) * width]
    return [int.from_bytes(raw[i * width:(i + 1) * width], "little", signed=True) for i in range(len(arr))]


# ---- temporal types ---------------------------------------------------------------------------------------------------------
I32_MIN, I32_MAX, I64_MIN, I64_MAX = -2**31, 2**31 - 1, -2**63, 2**63 - 1
I32_EDGES: List[int] = [I32_MIN, I32_MIN + 1, -2**16, -1, 0, 1, 2**16, I32_MAX - 1, I32_MAX]
# the last rows before INT_MAX - 1: pairs that differ in the low word only (by 1, by its top bit) and in the high word only
# (by 1, by its top bit -- a negative value)
I64_EDGES: List[int] = [I64_MIN, I64_MIN + 1, -2**32, -2**31 - 1, -2**16, -1, 0, 1, 2**16, 2**31 - 1, 2**31, 2**32 - 1, 2**32,
                        0x0000000500000007, 0x0000000500000008, 0x0000000580000007, 0x0000000600000007,
                        0x0000000500000007 - 2**63, I64_MAX - 1, I64_MAX]

# every DataType csrc/plan.cpp's opaque_compare_class names: (id, type)
TEMPORAL_TYPES: List[Tuple[str, pa.DataType]] = [
    ("date32", pa.date32()), ("time32_s", pa.time32("s")), ("time32_ms", pa.time32("ms")),
    ("date64", pa.date64()), ("time64_us", pa.time64("us")), ("time64_ns", pa.time64("ns")),
] + [(f"timestamp_{u}{'_utc' if tz else ''}", pa.timestamp(u, tz=tz)) for u in ("s", "ms", "us", "ns") for tz in (None, "UTC")] \
  + [(f"duration_{u}", pa.duration(u)) for u in ("s", "ms", "us", "ns")]


def temporal_edges(typ: pa.DataType) -> List[int]:
    return I32_EDGES if typ.bit_width == 32 else I64_EDGES


def temporal_array(values: Sequence[int], typ: pa.DataType, valid=None) -> pa.Array:
    """raw values (a Time32 outside the day, a Timestamp outside datetime's range: Arrow does not validate them)"""
    data = np.array(values, dtype=np.int32 if typ.bit_width == 32 else np.int64)
    nulls = 0 if valid is None else int(len(values) - np.count_nonzero(valid))
    return pa.Array.from_buffers(typ, len(values), [validity_buffer(valid), pa.py_buffer(data.tobytes())], null_count=nulls)


def pair_table(edges: Sequence[int]) -> List[Tuple[int, int]]:
    """all ordered pairs of the table"""
    return [(a, b) for a in edges for b in edges]


def pair_batch_rows(edges: Sequence[int], shift: int = 37) -> List[Tuple[int, int]]:
    """the pair batch of the GPU tier: all ordered pairs, the same pairs rotated by `shift` rows -- each pair at two lane
    positions -- and one more row when that makes a multiple of 64, so the last wave is a partial one"""
    pairs = pair_table(edges)
    rows = pairs + pairs[shift:] + pairs[:shift]
    if len(rows) % 64 == 0:
        rows.append(pairs[0])
    return rows


# ---- Utf8 -> Boolean --------------------------------------------------------------------------------------------------------
# Unicode White_Space = Rust's char::is_whitespace
WHITE_SPACE: List[int] = [0x0009, 0x000A, 0x000B, 0x000C, 0x000D, 0x0020, 0x0085, 0x00A0, 0x1680, 0x2000, 0x2001, 0x2002, 0x2003,
                          0x2004, 0x2005, 0x2006, 0x2007, 0x2008, 0x2009, 0x200A, 0x2028, 0x2029, 0x202F, 0x205F, 0x3000]
_WS_BYTES = [chr(c).encode("utf-8") for c in WHITE_SPACE]
TRUE_SPELLINGS = (b"t", b"tr", b"tru", b"true", b"y", b"ye", b"yes", b"on", b"1")
FALSE_SPELLINGS = (b"f", b"fa", b"fal", b"fals", b"false", b"n", b"no", b"of", b"off", b"0")


def utf8_to_bool(b: bytes) -> Optional[bool]:
    """arrow-cast 53 cast_utf8_to_boolean on one (valid UTF-8) value; None = NULL.  A byte suffix that equals a character's
    encoding IS that character in valid UTF-8, so the trailing strip is exact on bytes"""
    again = True
    while again:
        again = False
        for w in _WS_BYTES:
            if b[:len(w)] == w:
                b, again = b[len(w):], True
    again = True
    while again:
        again = False
        for w in _WS_BYTES:
            if len(b) >= len(w) and b[len(b) - len(w):] == w:
                b, again = b[:len(b) - len(w)], True
    low = bytes(c + 32 if 0x41 <= c <= 0x5A else c for c in b)
    if low in TRUE_SPELLINGS:
        return True
    if low in FALSE_SPELLINGS:
        return False
    return None


def _case_mixes(s: bytes) -> List[bytes]:
    out = []
    for bits in itertools.product((0, 1), repeat=len(s)):
        out.append(bytes(c - 32 if up and 0x61 <= c <= 0x7A else c for c, up in zip(s, bits)))
    return _unique(out)


def _u(*cps: int) -> bytes:
    return "".join(chr(c) for c in cps).encode("utf-8")


# not White_Space, but in a wrong table it would be: the separators Python strips, the zero-width and formerly-space
# characters, NUL
NOT_WS_TABLE = [0x001C, 0x001D, 0x001E, 0x001F, 0x200B, 0x180E, 0x2060, 0xFEFF, 0x0000]
# not White_Space, but a scan that walks backwards over continuation bytes, or matches trailing bytes alone, would take them
# for it: they share their last byte or two with U+00A0 (C2 A0), U+0085 (C2 85), U+1680 (E1 9A 80), U+2000 (E2 80 80),
# U+2028 (E2 80 A8), U+3000 (E3 80 80), U+205F (E2 81 9F)
NOT_WS_BYTES = [0x00E0, 0x0145, 0x10A0, 0x1A80, 0x2080, 0x20A8, 0x3040, 0x205E, 0x2030]
PAD_WORDS = (b"true", b"F", b"1", b"off", b"no")
PAD_LENGTHS = (1, 63, 64, 65, 1000)


def _mixed_run(n: int) -> bytes:
    """n white-space characters, 1-, 2- and 3-byte ones in turn"""
    cycle = [0x20, 0xA0, 0x2003, 0x09, 0x85, 0x3000, 0x0D, 0x1680, 0x205F]
    return _u(*[cycle[i % len(cycle)] for i in range(n)])


def _build_word_table() -> List[bytes]:
    words: List[bytes] = []
    spellings = TRUE_SPELLINGS + FALSE_SPELLINGS
    for s in spellings:                                              # every spelling in every case mix
        words += _case_mixes(s)
    for s in spellings:                                              # one byte appended, removed, replaced by a neighbour
        words += [s + bytes([c]) for c in b"aeflnorstuyEX012-."]
        words += [s[:i] + s[i + 1:] for i in range(len(s))]
        words += [s[:i] + bytes([s[i] + d]) + s[i + 1:] for i in range(len(s)) for d in (-1, 1)]
        words += [bytes([c]) + s for c in b"a-+0"]
    words += [b"treu", b"yess", b"falsee", b"o", b"00", b"2", b"-1", b"+1", b"01", b"10", b"1.0", b"tRuE!", b"nO.", b"oN", b"oF", b"Of", b"OFf"]
    words += [b"falsee", b"falsey", b"truetrue", b"yesyes", b"ffffff", b"FALSEFALSE", b"a" * 100, b"t" * 64, b"true" * 300]   # six bytes and longer
    for c in WHITE_SPACE:                                            # every White_Space character around a spelling
        w, nxt = _u(c), _u(WHITE_SPACE[(WHITE_SPACE.index(c) + 1) % len(WHITE_SPACE)])
        for s in PAD_WORDS:
            words += [w + s, s + w, w + s + w, w + w + s + w + w, nxt + w + s + w + nxt + w]
        words += [b"t" + w + b"rue", b"o" + w + b"n", b"on" + w + b"n", b"fal" + w + w + b"se"]           # interior: not trimmed
        words += [w, w + w, w + nxt + w]                                                                  # nothing else
    words += [b"", b"t rue", b"on\tn", b"tr\nue", b"1 1", b"y e s", _u(0x2028) + b"y" + _u(0x85), b"\x0bNo\x0c", b"\r\n\tYeS \n"]
    for n in PAD_LENGTHS:                                            # long runs around `1`
        for pad in (b" " * n, _u(0xA0) * n, _u(0x2003) * n, _mixed_run(n)):
            words += [pad + b"1", b"1" + pad, pad + b"1" + pad, pad]
    words += [_mixed_run(1000) + b"falsee" + _mixed_run(1000), _mixed_run(999) + b"x" + _mixed_run(1000) + b"1"]
    for c in NOT_WS_TABLE + NOT_WS_BYTES:                            # lookalikes, before and after a valid spelling
        w = _u(c)
        for s in (b"true", b"0"):
            words += [w + s, s + w, w + s + w, b" " + w + s, s + w + b" ", w + b" " + s, s + b" " + w, _u(0x2003) + s + w + _u(0x2003)]
        words += [w, w + w, b" " + w + b" "]
    for s in spellings:                                              # NUL bytes behind a spelling, up to five bytes in all
        words += [s + b"\x00" * k for k in range(1, 6 - len(s))]
    # non-ASCII lookalikes of letters: fullwidth, long s, dotted capital I, Kelvin sign (Python's lower() folds the last three)
    words += [_u(0xFF54, 0xFF52, 0xFF55, 0xFF45), _u(0xFF34, 0xFF32, 0xFF35, 0xFF25), b"ye" + _u(0x017F), b"YE" + _u(0x017F), _u(0x0130),
              b"fal" + _u(0x017F) + b"e", b"tru" + _u(0xE9), _u(0xE9), b"t" + _u(0x0300), _u(0xFF11), _u(0x0661), _u(0x212A),
              _u(0x1D7CF), b"o" + _u(0xFF4E), b"n" + _u(0x00D6)]
    return _unique(words)


BOOL_WORDS: List[bytes] = _build_word_table()
# (bytes, expected): True / False / None (NULL)
BOOL_WORD_TABLE: List[Tuple[bytes, Optional[bool]]] = [(w, utf8_to_bool(w)) for w in BOOL_WORDS]
assert 1000 < len(BOOL_WORD_TABLE) < 5000
for _w in BOOL_WORDS:
    _w.decode("utf-8")   # every row is valid UTF-8


def utf8_array(values: Sequence[bytes], valid=None, trailing: bytes = b"") -> pa.Array:
    """a Utf8 column from raw bytes; `trailing` bytes follow the last value in the data buffer"""
    offs = np.zeros(len(values) + 1, np.int32)
    np.cumsum([len(v) for v in values], out=offs[1:])
    nulls = 0 if valid is None else int(len(values) - np.count_nonzero(valid))
    return pa.Array.from_buffers(pa.utf8(), len(values), [validity_buffer(valid), pa.py_buffer(offs.tobytes()), pa.py_buffer(b"".join(values) + trailing)],
                                 null_count=nulls)


def bool_result(values: Sequence[Optional[bool]]) -> pa.Array:
    return pa.array(list(values), pa.bool_())
