"""Generators and the expected result for the Utf8 movement of the filter (test_utf8_reference.py checks this module on the
host, test_gpu_utf8_edges.py runs the kernels against it).  numpy only.

Every byte of a generated column identifies its place: byte k of row r is 0x21 + ((r * 131 + k * 7) % 94), printable ASCII, so
neighbouring rows differ and so do neighbouring 4-byte and 16-byte chunks of one row -- a byte written one place off, a lost
1-3-byte tail or a chunk taken from the row next door changes the output.  (Strings of one repeated letter cannot show any of
these.)  The bytes in front of the first offset (`lead`) are spaces, 0x20, which no row contains.

Thresholds of the device code the profiles and selections are placed around (kernels.hip):
  column rule   byte span <= 24 x rows: bytes move inside filter_fused_kernel / utf8_filter_kernel; above: utf8_copy_kernel
  group rule    bytes of a 64-row group's selected rows > 24 x their count: the group goes through copy_rows_wide
  row length    4 / 8 / 12 / 16 (the 4- and 8-byte accesses of the short path), len & 3 (the byte tail), len & 15 and 128
                (copy_rows_wide: 16-byte chunks, eight lanes per row, 128 bytes per pass)
  selection     copy_rows_wide takes 16 rows per step (15 / 16 / 17 selected rows); utf8_copy_kernel copies run by run
                unless runs x 4 > selected rows (runs of three rows: row by row; of four: by run)
  run bytes     16 (one chunk per lane), 1024 (one chunk per lane and pass), 3088 (lane 0 enters the four-chunk loop), 4096
"""
from __future__ import annotations

from typing import Callable, Dict, NamedTuple, Optional, Tuple

import numpy as np
import pyarrow as pa

GROUP = 64            # rows per group: one wave, one word of the selection bitmap
TILE = 16384          # rows of the largest tile kind
N_GPU = 3 * TILE + 101
SPIKE = 70_000
RUN_TARGETS = (1023, 1024, 1025, 3087, 3088, 3089, 4095, 4096, 4097, 8200)


# ---- columns -----------------------------------------------------------------------------------------------------------
def make_utf8(lengths, valid=None, lead: int = 0) -> pa.StringArray:
    """A Utf8 array of the given row lengths whose offsets begin at `lead`.  `valid`: bool per row (None: no bitmap); a null
    row keeps the bytes its length asks for."""
    lengths = np.asarray(lengths, dtype=np.int64)
    n = len(lengths)
    ends = np.cumsum(lengths)
    total = int(ends[-1]) if n else 0
    assert lead + total < 2**31
    offsets = np.empty(n + 1, dtype=np.int32)
    offsets[0] = lead
    offsets[1:] = lead + ends
    row = np.repeat(np.arange(n, dtype=np.int64), lengths)
    k = np.arange(total, dtype=np.int64) - np.repeat(ends - lengths, lengths)
    data = np.empty(lead + total, dtype=np.uint8)
    data[:lead] = 0x20
    data[lead:] = 0x21 + (row * 131 + k * 7) % 94
    bitmap, nulls = None, 0
    if valid is not None:
        valid = np.asarray(valid, dtype=bool)
        assert len(valid) == n
        bitmap = pa.py_buffer(np.packbits(valid, bitorder="little").tobytes())
        nulls = int(n - valid.sum())
    return pa.StringArray.from_buffers(n, pa.py_buffer(offsets.tobytes()), pa.py_buffer(data.tobytes()), bitmap, nulls, 0)


def utf8_parts(array: pa.Array) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(offsets [len + 1] as stored, the whole data buffer, validity as bool per row) of a Utf8 array, slice offset applied.
    The offsets buffer must hold all len + 1 offsets, also for an array of no rows."""
    n, off = len(array), array.offset
    bufs = array.buffers()
    assert bufs[1] is not None and bufs[1].size >= 4 * (off + n + 1), \
        f"offsets buffer of {0 if bufs[1] is None else bufs[1].size} bytes for {n} rows at offset {off}"
    offsets = np.frombuffer(bufs[1], dtype=np.int32, count=n + 1, offset=4 * off)
    data = np.frombuffer(bufs[2], dtype=np.uint8) if len(bufs) > 2 and bufs[2] is not None else np.zeros(0, dtype=np.uint8)
    if bufs[0] is None:
        valid = np.ones(n, dtype=bool)
    else:
        valid = np.unpackbits(np.frombuffer(bufs[0], dtype=np.uint8), bitorder="little")[off:off + n].astype(bool)
    return offsets, data, valid


def expected_filter(array: pa.Array, keep) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """What filtering `array` by the bool mask `keep` gives: (offsets rebased to 0 [kept + 1], the kept rows' bytes one after
    the other, the kept rows' validity)."""
    keep = np.asarray(keep, dtype=bool)
    offsets, data, valid = utf8_parts(array)
    starts = offsets[:-1].astype(np.int64)[keep]
    lens = np.diff(offsets.astype(np.int64))[keep]
    out = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(lens, out=out[1:])
    idx = np.repeat(starts - out[:-1], lens) + np.arange(out[-1], dtype=np.int64)
    return out.astype(np.int32), data[idx], valid[keep]


# ---- length profiles -----------------------------------------------------------------------------------------------------
class Profile(NamedTuple):
    lengths: Callable[[int], np.ndarray]   # n -> row lengths
    side: str                              # "short": byte span <= 24 x rows at N_GPU rows, "long": above


def _lane(n):
    return np.arange(n, dtype=np.int64) % GROUP


def _group(n):
    return np.arange(n, dtype=np.int64) // GROUP


def _const(L):
    return lambda n: np.full(n, L, dtype=np.int64)


GROUP24_EVEN = 24 * GROUP       # bytes of an even group: lanes cycle through 20, 28, 23, 25
GROUP24_ODD = 24 * GROUP + 1    # bytes of an odd group: 24 everywhere, one 25-byte row in lane 5


def _group24(first_group_empty):
    def lengths(n):
        lane, grp = _lane(n), _group(n)
        out = np.where(grp % 2 == 0, np.array([20, 28, 23, 25])[lane % 4], np.where(lane == 5, 25, 24))
        if first_group_empty:   # takes 24 x 64 bytes off the total: the column comes to lie below 24 x rows
            out[:GROUP] = 0
        return out
    return lengths


def spike_rows(n, four):
    """the rows of the 70 000-byte strings: lane 0, lane 63 and a lane in mid-group, each in a tile of its own (tiles shrink
    with n below three full tiles); `four`: the mid-group one is followed by three more"""
    tile = TILE if n >= 3 * TILE else max(GROUP, n // 3 // GROUP * GROUP)
    rows = [GROUP, tile + 2 * GROUP + 63, 2 * tile + 3 * GROUP + 30]
    if four:
        rows += [rows[2] + 1, rows[2] + 2, rows[2] + 3]
    return [r for r in rows if r < n]


def _spike(four):
    def lengths(n):
        out = np.zeros(n, dtype=np.int64)
        out[spike_rows(n, four)] = SPIKE
        return out
    return lengths


def _runs_all(n):
    """under `all` a group is one run: group g holds RUN_TARGETS[g % 10] bytes, T // 64 per row and one more in the first
    T % 64 lanes"""
    t = np.array(RUN_TARGETS)[_group(n) % len(RUN_TARGETS)]
    return t // GROUP + (_lane(n) < t % GROUP)


RUNS4_GROUP_STRIDE = 16   # every 16th group carries the runs (the others hold 30-byte rows: the column stays small)


def _runs_runs4(n):
    """under `runs4` (lanes 5 j .. 5 j + 3 kept) run j of every 16th group g holds RUN_TARGETS[(g / 16 + j) % 10] bytes:
    T // 4 per row and one more in the first T % 4 rows of the run; the gap rows hold 5 bytes, every other group 30 per row"""
    lane, grp = _lane(n), _group(n)
    t = np.array(RUN_TARGETS)[(grp // RUNS4_GROUP_STRIDE + lane // 5) % len(RUN_TARGETS)]
    pat = np.where(lane % 5 == 4, 5, t // 4 + (lane % 5 < t % 4))
    return np.where(grp % RUNS4_GROUP_STRIDE == 0, pat, 30)


def _mixed(n):
    """seven groups of 0..8-byte rows, then one of 90..129-byte rows: both kinds inside every 512 rows"""
    lane, grp = _lane(n), _group(n)
    return np.where(grp % 8 == 7, 90 + lane % 40, lane % 9)


LENGTH_PROFILES: Dict[str, Profile] = {"cycle41": Profile(lambda n: np.arange(n, dtype=np.int64) % 41, "short")}
for _L in (0, 1, 2, 3, 4, 7, 8, 11, 12, 15, 16, 17, 23, 24, 25, 33, 127, 128, 129, 143, 255, 257):
    LENGTH_PROFILES[f"const{_L}"] = Profile(_const(_L), "short" if _L <= 24 else "long")
LENGTH_PROFILES.update({
    "group24_short": Profile(_group24(True), "short"),
    "group24_long": Profile(_group24(False), "long"),
    "spike": Profile(_spike(False), "short"),
    "spike4": Profile(_spike(True), "short"),
    "runs3088_all": Profile(_runs_all, "long"),
    "runs3088_runs4": Profile(_runs_runs4, "long"),
    "mixed": Profile(_mixed, "short"),
})


# ---- selections ----------------------------------------------------------------------------------------------------------
def _runs(k):   # k kept, one dropped, restarting with every group: runs3 -> 16 runs of 48 rows (row by row in
    return lambda n: _lane(n) % (k + 1) != k   # utf8_copy_kernel), runs4 -> 13 of 52, runs5 -> 11 of 54 (by run)


def _random(p):
    return lambda n: np.random.default_rng(int(p * 100) + 7).random(n) < p


SCATTER = 37   # odd: lane -> lane * 37 % 64 is a permutation of the lanes


SELECTIONS: Dict[str, Callable[[int], np.ndarray]] = {
    "none": lambda n: np.zeros(n, dtype=bool),
    "all": lambda n: np.ones(n, dtype=bool),
    "lane0": lambda n: _lane(n) == 0,
    "lane63": lambda n: _lane(n) == 63,
    "alternate": lambda n: _lane(n) % 2 == 0,
    "runs3": _runs(3), "runs4": _runs(4), "runs5": _runs(5),
}
for _c in (1, 8, 15, 16, 17, 63):
    SELECTIONS[f"count{_c}"] = (lambda c: lambda n: _lane(n) < c)(_c)                              # the first c rows of every group
    SELECTIONS[f"scatter{_c}"] = (lambda c: lambda n: _lane(n) * SCATTER % GROUP < c)(_c)          # c rows of every group, spread out
SELECTIONS.update({
    "tiles_off": lambda n: (np.arange(n) // TILE) % 2 == 1,
    "first_and_last_row": lambda n: np.isin(np.arange(n), [0, n - 1]),
    "random02": _random(0.02), "random50": _random(0.5), "random98": _random(0.98),
})


# ---- comparisons -----------------------------------------------------------------------------------------------------------
_CMP = {"Eq": lambda a, b: a == b, "NotEq": lambda a, b: a != b, "Lt": lambda a, b: a < b,
        "LtEq": lambda a, b: a <= b, "Gt": lambda a, b: a > b, "GtEq": lambda a, b: a >= b}
COMPARE_OPS = tuple(_CMP)


def compare_bytes(op: str, a: Optional[bytes], b: Optional[bytes]) -> Optional[bool]:
    """`a op b` on byte strings: unsigned lexicographic order, a prefix before its extensions; null in, null out"""
    if a is None or b is None:
        return None
    return _CMP[op](a, b)


_S65 = bytes(0x30 + i % 10 for i in range(65))
_S300 = bytes(0x41 + i % 26 for i in range(300))
COMPARE_TABLE = (
    b"", b"a", b"a\x00", b"a\x00b", b"ab", b"b", b"B",
    b"\x7f", b"\x80", b"\xff",                                               # 80 and ff alone are not UTF-8: column against column only
    "é".encode(), "\uff5e".encode(), "\U00010000".encode(),             # c3 a9 / ef bd 9e / f0 90 80 80
    _S65, _S65[:64], _S65[:64] + b"Z",                                       # a prefix and its extension; byte 64 differs
    _S300, _S300[:299] + b"!",                                               # only the last of 300 bytes differs
)


def is_utf8(b: bytes) -> bool:
    try:
        b.decode("utf-8")
        return True
    except UnicodeDecodeError:
        return False


def binary_column(values, lead: int = 0) -> pa.StringArray:
    """a Utf8 array holding the given byte strings as they are (None: null), whether or not they are valid UTF-8"""
    n = len(values)
    lens = np.array([0 if v is None else len(v) for v in values], dtype=np.int64)
    offsets = np.zeros(n + 1, dtype=np.int32)
    offsets[0] = lead
    offsets[1:] = lead + np.cumsum(lens)
    data = b" " * lead + b"".join(v for v in values if v is not None)
    bitmap, nulls = None, 0
    if any(v is None for v in values):
        valid = np.array([v is not None for v in values])
        bitmap, nulls = pa.py_buffer(np.packbits(valid, bitorder="little").tobytes()), int(n - valid.sum())
    return pa.StringArray.from_buffers(n, pa.py_buffer(offsets.tobytes()), pa.py_buffer(data), bitmap, nulls, 0)


def compare_pairs(n: int):
    """(a values, b values): COMPARE_TABLE crossed with itself, repeated up to n rows"""
    t = len(COMPARE_TABLE)
    i = np.arange(n) % (t * t)
    return [COMPARE_TABLE[k] for k in i // t], [COMPARE_TABLE[k] for k in i % t]
