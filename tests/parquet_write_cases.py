"""Tables and shape builders for the page-encoder tests: the CPU test of the page reader (tests/test_parquet_unpage.py, on
files pyarrow writes) and the GPU suite (tests/test_gpu_parquet_write_edges.py, on files csrc/parquet_write.* writes) take
their inputs from here.  Strings and shapes are functions of the row number; `values()` and the 30 % validity are drawn
from fixed seeds.

The encoder's units, which the shapes are aligned with: the 64-lane prefix, the 256-row step, the 4096-row block whose base
comes from pw_scan_kernel, and the page (parquet_page_rows = 4096 in these tests, so N rows make a first, two middle and a
ragged last page)."""
from __future__ import annotations

import numpy as np
import pyarrow as pa

PAGE_ROWS = 4096
N = 3 * PAGE_ROWS + 5
TYPES = {"i32": pa.int32(), "i64": pa.int64(), "f32": pa.float32(), "f64": pa.float64(), "flag": pa.bool_(), "s": pa.utf8()}
EDGE_ROWS = (63, 64, 255, 256, 4095, 4096, N - 1)

# ---- strings whose every byte depends on its row and its position ------------------------------------------------------------
ALPHABET = 95            # printable ASCII 0x20 .. 0x7e; 95 is coprime to 16, the chunk pw_encode_kernel<0> moves, and to 7
STRING_LENGTHS = list(range(146)) + [255, 256, 257, 4095, 4096, 4097, 70_000] + list(range(21))
LONG_AT = 146            # rows [LONG_AT, LONG_AT + 7) of STRING_LENGTHS are the long ones


def _mix(i: np.ndarray) -> np.ndarray:
    """a 64-bit mixer (multiply / xor-shift) of the position, so that a long string does not repeat itself"""
    x = i.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    x ^= x >> np.uint64(32)
    x *= np.uint64(0xD6E8FEB86659FD93)
    x ^= x >> np.uint64(32)
    return (x % np.uint64(ALPHABET)).astype(np.int64)


def text_bytes(rows, lengths) -> tuple:
    """(offsets int32, data uint8) of strings: byte i of row r is 0x20 + (i + 7 * r + mix(i)) % 95.  Rows r and r + 1 differ
    in every byte they share; no two 16-byte chunks of one string are equal (checked up to 70 000 bytes by
    tests/test_parquet_unpage.py), whatever their distance"""
    rows = np.asarray(rows, dtype=np.int64)
    lengths = np.asarray(lengths, dtype=np.int64)
    offs = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum(lengths, out=offs[1:])
    assert offs[-1] < 2**31
    r = np.repeat(rows, lengths)
    i = np.arange(offs[-1], dtype=np.int64) - np.repeat(offs[:-1], lengths)
    data = (0x20 + (i + 7 * r + _mix(i)) % ALPHABET).astype(np.uint8)
    return offs.astype(np.int32), data


def text(row: int, length: int) -> str:
    return text_bytes([row], [length])[1].tobytes().decode("ascii")


def packed(valid) -> pa.Buffer:
    return pa.py_buffer(np.packbits(np.asarray(valid, dtype=bool), bitorder="little").tobytes())


def text_array(lengths, valid=None, first_row: int = 0, bitmap: bool = False) -> pa.Array:
    """Utf8 array of text(first_row + k, lengths[k]); the bytes of a null row stay in the data buffer (a writer that looks
    under a null copies them).  bitmap=True keeps a validity buffer even when no row is null"""
    n = len(lengths)
    offs, data = text_bytes(first_row + np.arange(n), lengths)
    nulls = 0 if valid is None else int(n - np.count_nonzero(valid))
    vbuf = packed(valid) if valid is not None and (nulls or bitmap) else None
    return pa.StringArray.from_buffers(n, pa.py_buffer(offs.tobytes()), pa.py_buffer(data.tobytes()), vbuf, nulls if nulls or not bitmap else -1)


def string_shapes(n: int = N) -> pa.Table:
    """the string columns of the issue, n rows each: the length ladder at the front, then lengths that keep cycling through
    0 .. 145 (so the ladder's strings also meet every alignment behind the 70 000-byte one)"""
    lengths = np.array(STRING_LENGTHS + [(k * 37) % 146 for k in range(n - len(STRING_LENGTHS))], dtype=np.int64)
    valid = np.arange(n) % 5 != 2
    valid[LONG_AT:LONG_AT + 7] = True
    valid[[LONG_AT - 1, LONG_AT + 3, LONG_AT + 7]] = False   # nulls before, between (the 4095-byte row) and after the long strings
    under = valid.copy()                 # ... and the 70 000 bytes themselves under a null, valid rows on both sides
    under[LONG_AT + 6] = False
    under[[LONG_AT + 5, LONG_AT + 7]] = True
    third = np.arange(n) % 3
    return pa.table({
        "ladder": text_array(lengths),
        "ladder_nulls": text_array(lengths, valid),
        "ladder_long_under_null": text_array(lengths, under),
        "empty": text_array(np.zeros(n, dtype=np.int64)),
        "empty_or_null": text_array(np.zeros(n, dtype=np.int64), third != 1),
        "short_empty_null": text_array(np.where(third == 0, 0, 3), third != 1),
        "all_null": text_array((np.arange(n) * 7) % 40, np.zeros(n, dtype=bool)),
    })


# ---- values of every type ----------------------------------------------------------------------------------------------------
def values(name: str, n: int, seed: int = 0):
    """n values of column kind `name` as numpy (Utf8: lengths for text_array).  Floats carry NaNs of both signs with
    payloads, signed zeros, infinities and subnormals"""
    rng = np.random.default_rng(seed + sum(map(ord, name)))
    if name == "i32":
        return rng.integers(-2**31, 2**31, n).astype(np.int32)
    if name == "i64":
        return rng.integers(-2**63, 2**63, n, dtype=np.int64)
    if name == "f32":
        v = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)           # any bit pattern
        v[::11] = np.array([0x7FC00001, 0xFFC12345, 0x80000000, 0, 0x7F800000, 0xFF800000, 1, 0x80000001], dtype=np.uint32)[np.arange(len(v[::11])) % 8]
        return v.view(np.float32)
    if name == "f64":
        v = rng.integers(0, 2**64, n, dtype=np.uint64)
        v[::11] = np.array([0x7FF8000000000001, 0xFFF8123456789ABC, 1 << 63, 0, 0x7FF << 52, 0xFFF << 52, 1, (1 << 63) | 1], dtype=np.uint64)[np.arange(len(v[::11])) % 8]
        return v.view(np.float64)
    if name == "flag":
        return rng.random(n) < 0.4
    if name == "s":
        return (np.arange(n) * 13) % 23
    raise KeyError(name)


def column(name: str, n: int, valid=None, seed: int = 0, bitmap: bool = False, first_row: int = 0) -> pa.Array:
    """`valid`: None (no validity buffer) or a bool array; what lies under a null is kept as drawn"""
    v = values(name, n, seed)
    if name == "s":
        return text_array(v, valid, first_row, bitmap)
    nulls = 0 if valid is None else int(n - np.count_nonzero(valid))
    vbuf = packed(valid) if valid is not None and (nulls or bitmap) else None
    data = packed(v) if name == "flag" else pa.py_buffer(v.tobytes())
    return pa.Array.from_buffers(TYPES[name], n, [vbuf, data], nulls if nulls or not bitmap else -1)   # (-1: pyarrow keeps the bitmap)


def typed_batch(n: int, valid=None, nullable: bool = True, seed: int = 0, bitmap: bool = False) -> pa.RecordBatch:
    """one column of each of the six types under the same validity"""
    cols = [column(k, n, valid, seed, bitmap) for k in TYPES]
    return pa.RecordBatch.from_arrays(cols, schema=pa.schema([pa.field(k, t, nullable) for k, t in TYPES.items()]))


# ---- validity shapes ---------------------------------------------------------------------------------------------------------
def thirty_percent(n: int, seed: int = 9) -> np.ndarray:
    return np.random.default_rng(seed).random(n) >= 0.3


def page1_null(n: int = N) -> np.ndarray:
    v = thirty_percent(n, 10)
    v[PAGE_ROWS:2 * PAGE_ROWS] = False
    v[PAGE_ROWS - 1:PAGE_ROWS] = True              # values right up to the empty page ...
    v[2 * PAGE_ROWS:2 * PAGE_ROWS + 1] = True      # ... and right behind it
    return v


def validity_shapes(n: int = N) -> dict:
    """name -> (valid or None, nullable, keep a bitmap without nulls)"""
    r = np.arange(n)
    edges = np.isin(r, EDGE_ROWS)
    blocks01 = thirty_percent(n, 11)
    blocks01[:PAGE_ROWS] = False
    blocks01[PAGE_ROWS:2 * PAGE_ROWS] = True
    blocks10 = thirty_percent(n, 12)
    blocks10[:PAGE_ROWS] = True
    blocks10[PAGE_ROWS:2 * PAGE_ROWS] = False
    return {
        "bitmap_all_valid": (np.ones(n, dtype=bool), True, True),
        "all_null": (np.zeros(n, dtype=bool), True, False),
        "only_row_0": (r == 0, True, False),
        "only_last_row": (r == n - 1, True, False),
        "edge_rows": (edges, True, False),
        "all_but_edge_rows": (~edges, True, False),
        "block0_null_block1_valid": (blocks01, True, False),
        "block0_valid_block1_null": (blocks10, True, False),
        "page1_null": (page1_null(n), True, False),
        "random_30": (thirty_percent(n), True, False),
        "nullable_no_buffer": (None, True, False),
        "required": (None, False, False),
    }


VIEW_OFFSETS = (1, 7, 8, 9, 63, 64, 4095, 4096, 4097)
VIEW_PARENT_ROWS = N + 5000


def view_parent(offset: int, shape: str, n: int = N, rows: int = VIEW_PARENT_ROWS) -> pa.RecordBatch:
    """a parent of which rows [offset, offset + n) carry validity shape `shape` ("random_30", "page1_null", "no_nulls");
    the rows around the view have nulls, but the eight right behind it are valid (the last level byte's trailing bits).
    Six nullable columns and three required ones (Boolean, Int32, Utf8) that start at the same bit offset"""
    valid = thirty_percent(rows, 13 + offset)
    valid[:offset][::2] = False
    valid[offset:offset + n] = {"random_30": thirty_percent, "page1_null": page1_null, "no_nulls": lambda k: np.ones(k, dtype=bool)}[shape](n)
    valid[offset + n:offset + n + 8] = True
    valid[offset + n + 8:offset + n + 16] = False
    cols = [column(k, rows, valid, seed=offset) for k in TYPES] + [column(k, rows, None, seed=offset + 1) for k in ("flag", "i32", "s")]
    fields = [pa.field(k, t, True) for k, t in TYPES.items()] + [pa.field("req_" + k, TYPES[k], False) for k in ("flag", "i32", "s")]
    return pa.RecordBatch.from_arrays(cols, schema=pa.schema(fields))


ROW_GROUP_ROWS = (PAGE_ROWS + 1, 0, 1, 2 * PAGE_ROWS)


def row_group_batches(nullable: bool) -> list:
    out = []
    for g, n in enumerate(ROW_GROUP_ROWS):
        out.append(typed_batch(n, thirty_percent(n, 20 + g) if nullable and g != 2 else None, nullable, seed=30 + g))
    return out


# ---- statistics ----------------------------------------------------------------------------------------------------------------
def _spread(vals, n: int, dtype) -> np.ndarray:
    """the values of `vals` in turn over n rows"""
    return np.asarray(vals, dtype=dtype)[np.arange(n) % len(vals)]


def _bits32(*words) -> np.ndarray:
    return np.array(words, dtype=np.uint32).view(np.float32)


def _bits64(*words) -> np.ndarray:
    return np.array(words, dtype=np.uint64).view(np.float64)


def statistics_cases(n: int = N) -> pa.Table:
    """one column per case of the issue; every column has n rows.  What lies under a null is an extreme value, so that a
    reduction that looks under nulls is found out"""
    r = np.arange(n)
    last_only = r == n - 1
    some = thirty_percent(n, 40)
    cols = {}
    for nm, t, dt in (("i32", pa.int32(), np.int32), ("i64", pa.int64(), np.int64)):
        lo, hi = np.iinfo(dt).min, np.iinfo(dt).max
        cols[nm + "_only_min"] = pa.array(np.full(n, lo, dtype=dt))
        cols[nm + "_only_max"] = pa.array(np.full(n, hi, dtype=dt))
        cols[nm + "_min_and_max"] = pa.array(_spread([hi, lo, hi], n, dt))
        cols[nm + "_only_max_nulls"] = pa.Array.from_buffers(t, n, [packed(some), pa.py_buffer(np.where(some, hi, lo).astype(dt).tobytes())], int(n - some.sum()))
        cols[nm + "_only_min_nulls"] = pa.Array.from_buffers(t, n, [packed(some), pa.py_buffer(np.where(some, lo, hi).astype(dt).tobytes())], int(n - some.sum()))
        one = np.where(last_only, 42, _spread([lo, hi], n, dt)).astype(dt)
        cols[nm + "_single_value_last_row"] = pa.Array.from_buffers(t, n, [packed(last_only), pa.py_buffer(one.tobytes())], n - 1)
    for nm, t, dt, bits, tiny in (("f32", pa.float32(), np.float32, _bits32, float(np.float32(1e-45))), ("f64", pa.float64(), np.float64, _bits64, 5e-324)):
        top = 31 if dt == np.float32 else 63
        w = np.uint32 if dt == np.float32 else np.uint64
        exp_all = (0xFF << 23) if dt == np.float32 else (0x7FF << 52)
        qnan, nnan = bits(exp_all | (1 << (top - 9)) | 0x1234), bits((1 << top) | exp_all | (1 << (top - 9)) | 0x4321)
        snan = bits(exp_all | 0x55)
        nans = np.concatenate([qnan, nnan, snan])
        cols[nm + "_only_pos_zero"] = pa.array(np.zeros(n, dtype=dt))
        cols[nm + "_only_neg_zero"] = pa.array(np.full(n, -0.0, dtype=dt))
        cols[nm + "_pos_zero_nan"] = pa.array(np.concatenate([_spread([0.0], n, dt)[:-3], nans]))
        cols[nm + "_zeros_and_subnormals"] = pa.array(_spread([-0.0, 0.0, tiny, -tiny], n, dt))
        cols[nm + "_infinities"] = pa.array(_spread([1.5, np.inf, -2.5, -np.inf, 0.0], n, dt))
        cols[nm + "_only_neg_inf"] = pa.array(np.full(n, -np.inf, dtype=dt))
        mixed = _spread([3.25, -7.5, 1e30, -1e-30], n, dt).copy()
        mixed.view(w)[::7] = _spread(nans.view(w), len(mixed[::7]), w)
        cols[nm + "_nans_among_values"] = pa.array(mixed)
        cols[nm + "_negative_values_only"] = pa.array(_spread([-3.0, -1e-30, -tiny, -1e30], n, dt))
        only_nan = _spread(nans.view(w), n, w).view(dt)
        cols[nm + "_only_nans_and_nulls"] = pa.Array.from_buffers(t, n, [packed(some), pa.py_buffer(np.where(some, only_nan, dt(1.0)).astype(dt).tobytes())], int(n - some.sum()))
        one = np.where(last_only, dt(-0.0), dt(9.0)).astype(dt)
        cols[nm + "_single_neg_zero_last_row"] = pa.Array.from_buffers(t, n, [packed(last_only), pa.py_buffer(one.tobytes())], n - 1)
    cols["flag_all_false"] = pa.array(np.zeros(n, dtype=bool))
    cols["flag_all_true"] = pa.array(np.ones(n, dtype=bool))
    cols["flag_mixed"] = pa.array(r % 3 == 1)
    cols["flag_all_null"] = pa.Array.from_buffers(pa.bool_(), n, [packed(np.zeros(n, dtype=bool)), packed(r % 2 == 0)], n)
    cols["flag_true_under_nulls"] = pa.Array.from_buffers(pa.bool_(), n, [packed(some), packed(~some)], int(n - some.sum()))
    cols["flag_single_true_last_row"] = pa.Array.from_buffers(pa.bool_(), n, [packed(last_only), packed(last_only)], n - 1)

    def words(ws, valid=None, first=None, last=None):
        ws = [ws[k % len(ws)] for k in range(n)]
        if first is not None:
            ws[0] = first
        if last is not None:
            ws[-1] = last
        return pa.array(ws, type=pa.utf8(), mask=None if valid is None else ~valid)
    k4096, k4097 = text(1, 4096), text(1, 4097)
    cols["s_empty_is_min"] = words(["b", "", "a"])
    cols["s_ties"] = words(["mm", "aa", "zz", "aa", "zz"])
    cols["s_shared_prefix"] = words(["ab\0", "abc", "ab", "ab\0"])
    cols["s_unsigned_bytes"] = words(["z", "é", "\U0001F600", "A"])
    cols["s_min_first_max_last"] = words(["m", "n", "o"], first="a", last="z")
    cols["s_max_first_min_last"] = words(["m", "n", "o"], first="z", last="a")
    cols["s_min_4096"] = words(["~~b", "~~c"], last=k4096)             # (text(1, .) starts with 0x27: between "\x1f" and "~")
    cols["s_max_4096"] = words(["\x1fa", "\x1fb"], first=k4096)
    cols["s_min_4097"] = words(["~~b", "~~c"], first=k4097)
    cols["s_max_4097"] = words(["\x1fa", "\x1fb"], last=k4097)
    cols["s_min_under_null"] = words(["m", "\x01", "\x7f", "q"], valid=r % 4 != 1)
    cols["s_single_value_last_row"] = words(["\x01", "\x7f"], valid=last_only, last="k")
    return pa.table(cols)


STATS_VIEW_OFFSETS = (5, 8)     # through pw_shift_bits_kernel / level bytes shared with the parent; N + 5 and N + 8 are no multiples of 8


def statistics_view_parent(offset: int, n: int = N) -> pa.RecordBatch:
    """rows [offset, offset + n) hold middling values; the valid rows directly before and behind them hold a smaller and a
    larger value.  The row behind the view lies in the validity byte of the view's last row, the row before it (offset 5) in
    that of its first"""
    rows = offset + n + 8
    inside = np.zeros(rows, dtype=bool)
    inside[offset:offset + n] = True
    valid = np.ones(rows, dtype=bool)
    valid[offset + 5::9] = False
    valid[[offset - 1, offset, offset + n - 1, offset + n]] = True
    lo_at, hi_at = offset - 1, offset + n

    def num(dt, mid_lo, mid_hi, lo, hi, under_nulls=True):
        v = np.where(np.arange(rows) % 2 == 0, mid_lo, mid_hi).astype(dt)
        v[:offset], v[offset + n:] = hi, lo
        v[lo_at], v[hi_at] = lo, hi
        if under_nulls:
            v[~valid] = lo
        return v
    s = ["g" if k % 2 else "p" for k in range(rows)]
    s[lo_at], s[hi_at] = "", "zzzz"
    flags = np.zeros(rows, dtype=bool)
    flags[~inside] = True
    arrays = {
        "i32": (pa.int32(), num(np.int32, -5, 7, -2**31, 2**31 - 1)),
        "i64": (pa.int64(), num(np.int64, -5, 7, -2**63, 2**63 - 1)),
        "f32": (pa.float32(), num(np.float32, -0.5, 2.5, -np.inf, np.inf)),
        "f64": (pa.float64(), num(np.float64, -0.5, 2.5, -np.inf, np.inf)),
    }
    cols, fields = [], []
    for k, (t, v) in arrays.items():
        cols.append(pa.Array.from_buffers(t, rows, [packed(valid), pa.py_buffer(v.tobytes())], int(rows - valid.sum())))
        fields.append(pa.field(k, t, True))
    cols.append(pa.Array.from_buffers(pa.bool_(), rows, [packed(valid), packed(flags)], int(rows - valid.sum())))
    fields.append(pa.field("flag", pa.bool_(), True))
    cols.append(pa.array(s, type=pa.utf8(), mask=~valid))
    fields.append(pa.field("s", pa.utf8(), True))
    cols.append(pa.array(num(np.int64, -5, 7, -2**63, 2**63 - 1, under_nulls=False)))
    fields.append(pa.field("req_i64", pa.int64(), False))
    cols.append(pa.array(s, type=pa.utf8()))
    fields.append(pa.field("req_s", pa.utf8(), False))
    return pa.RecordBatch.from_arrays(cols, schema=pa.schema(fields))
