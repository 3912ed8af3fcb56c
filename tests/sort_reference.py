"""Host reference of ORDER BY (tests only): every key type mapped to the same normalised unsigned keys the library
sorts by, `numpy.lexsort` (stable) over them with the null placement as a leading key, then the
rows taken.  Utf8 keys are ranked by Python's bytes order (bytewise, a proper prefix first)."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np
import pyarrow as pa

SIGN64 = np.uint64(1 << 63)
ALL64 = np.uint64(0xFFFFFFFFFFFFFFFF)

# (column, descending, nulls_first)
Key = Tuple[str, bool, bool]


def _fixed_raw(arr: pa.Array, width: int) -> np.ndarray:
    """the values buffer of `arr` (offset applied) as unsigned integers of `width` bytes"""
    dt = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[width]
    buf = arr.buffers()[1]
    return np.frombuffer(buf, dtype=dt, count=arr.offset + len(arr))[arr.offset:]


def _signed(raw: np.ndarray, width: int) -> np.ndarray:
    st = {1: np.int8, 2: np.int16, 4: np.int32, 8: np.int64}[width]
    return raw.view(st).astype(np.int64).view(np.uint64) ^ SIGN64


def _float(raw: np.ndarray, width: int) -> np.ndarray:
    u = raw.astype(np.uint64)
    bits = 8 * width
    sign = np.uint64(1 << (bits - 1))
    mask = np.uint64((1 << bits) - 1) if bits < 64 else ALL64
    return np.where((u & sign) != 0, ~u & mask, u | sign)


def value_words(arr: pa.Array) -> List[np.ndarray]:
    """the ascending order words of `arr`, most significant first (null rows: arbitrary)"""
    t = arr.type
    n = len(arr)
    if pa.types.is_boolean(t):
        return [np.asarray(arr.fill_null(False).to_numpy(zero_copy_only=False), dtype=np.uint64)]
    if pa.types.is_string(t):
        vals = [v.as_buffer().to_pybytes() if v.is_valid else b"" for v in arr]
        rank = {v: i for i, v in enumerate(sorted(set(vals)))}
        return [np.array([rank[v] for v in vals], dtype=np.uint64)]
    if pa.types.is_decimal(t):
        if t.bit_width <= 64:   # ordered as its signed integer
            return [_signed(_fixed_raw(arr, t.bit_width // 8), t.bit_width // 8)]
        w = np.frombuffer(arr.buffers()[1], dtype=np.uint64, count=2 * (arr.offset + n))[2 * arr.offset:].reshape(n, 2)
        return [w[:, 1] ^ SIGN64, w[:, 0].copy()]
    if pa.types.is_floating(t):
        width = t.bit_width // 8
        return [_float(_fixed_raw(arr, width), width)]
    if pa.types.is_unsigned_integer(t):
        return [_fixed_raw(arr, t.bit_width // 8).astype(np.uint64)]
    if pa.types.is_integer(t) or pa.types.is_temporal(t):
        width = t.bit_width // 8
        return [_signed(_fixed_raw(arr, width), width)]
    raise TypeError(f"no order for {t}")


def sort_indices(batch: pa.RecordBatch, keys: Sequence[Key]) -> np.ndarray:
    n = batch.num_rows
    words: List[np.ndarray] = []   # most significant first
    for name, desc, nulls_first in keys:
        arr = batch.column(batch.schema.get_field_index(name))
        valid = np.asarray(arr.is_valid().to_numpy(zero_copy_only=False), dtype=bool)
        flag = (valid == bool(nulls_first)).astype(np.uint64)
        words.append(flag)
        for w in value_words(arr):
            w = (~w if desc else w).copy()
            w[~valid] = 0
            words.append(w)
    if not words or n < 2:
        return np.arange(n)
    return np.lexsort(list(reversed(words)))


def join(batches: Sequence[pa.RecordBatch]) -> pa.RecordBatch:
    if len(batches) == 1:
        return batches[0]
    t = pa.Table.from_batches(list(batches)).combine_chunks()
    out = t.to_batches()
    return out[0] if out else batches[0].slice(0, 0)


def sort_batches(batches: Sequence[pa.RecordBatch], keys: Sequence[Key], limit: Optional[int] = None) -> pa.RecordBatch:
    b = join(batches)
    idx = sort_indices(b, keys)
    if limit is not None:
        idx = idx[:limit]
    return b.take(pa.array(idx, type=pa.int64()))


def sort_batch(batch: pa.RecordBatch, keys: Sequence[Key], limit: Optional[int] = None) -> pa.RecordBatch:
    return sort_batches([batch], keys, limit)


def keys_of(order_by, schema: pa.Schema) -> List[Key]:
    """sqlast.OrderByExpr (column keys) -> reference keys, SQL defaults resolved"""
    from chapterhouseqe_amd import sqlast as A
    out = []
    for o in order_by:
        e = o.expr
        name = e.ident.value if isinstance(e, A.Identifier) else e.idents[-1].value
        desc, nulls_first = o.sort_options()
        out.append((name, desc, nulls_first))
    return out
