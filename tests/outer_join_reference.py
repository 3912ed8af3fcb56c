"""Host reference of the join kinds (tests only), plain Python on top of tests/join_reference.py.

matches(l) is what `join_reference.join_indices` pairs with left row l (a null key matches nothing).  Per kind the
reference returns two row-id lists of one length, `None` standing for "no row":

  inner   the pairs, ascending by left row, then by right row
  left    for each left row ascending: its pairs, or (l, None) when it has none
  right   `left` with the sides exchanged: ascending by right row, then by left row; (None, r) for an unmatched right row
  full    the rows of `left`, then (None, r) for every right row no left row matches, ascending
  semi    (l,) for every left row with a match, ascending -- no right list
  anti    (l,) for every left row without one (a null key among them), ascending -- no right list

The expected batch is `Array.take` over index arrays that hold nulls; the fields of a padded side are forced nullable.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import pyarrow as pa

from . import join_reference as J
from . import sort_reference as R

KINDS = ["inner", "left", "right", "full", "semi", "anti"]
KIND_CODES = {"inner": 0, "left": 1, "right": 2, "full": 3, "semi": 4, "anti": 5}   # enum chq_join_kind

Ids = List[Optional[int]]


def _left_indices(left: pa.RecordBatch, right: pa.RecordBatch, keys: Sequence[J.KeyPair]) -> Tuple[Ids, Ids]:
    """LEFT from scratch: the dict of the right rows' keys, then every left row in order"""
    table = {}
    for j, k in enumerate(J._row_keys(right, [rk for _, rk in keys])):
        if k is not None:
            table.setdefault(k, []).append(j)
    lidx, ridx = [], []
    for i, k in enumerate(J._row_keys(left, [lk for lk, _ in keys])):
        hits = table.get(k, ()) if k is not None else ()
        for j in hits:
            lidx.append(i)
            ridx.append(j)
        if not hits:
            lidx.append(i)
            ridx.append(None)
    return lidx, ridx


def join_indices(left: pa.RecordBatch, right: pa.RecordBatch, keys: Sequence[J.KeyPair], kind: str) -> Tuple[Ids, Optional[Ids]]:
    assert keys, "there is no cross join"
    if kind == "inner":
        return J.join_indices(left, right, keys)
    if kind == "left":
        return _left_indices(left, right, keys)
    if kind == "right":
        ridx, lidx = _left_indices(right, left, [(rk, lk) for lk, rk in keys])
        return lidx, ridx
    if kind == "full":
        lidx, ridx = _left_indices(left, right, keys)
        matched = {j for j in ridx if j is not None}
        tail = [j for j in range(right.num_rows) if j not in matched]
        return lidx + [None] * len(tail), ridx + tail
    if kind in ("semi", "anti"):
        matched = set(J.join_indices(left, right, keys)[0])
        return [i for i in range(left.num_rows) if (i in matched) == (kind == "semi")], None
    raise ValueError(kind)


def padded_sides(kind: str) -> Tuple[bool, bool]:
    """(the left columns may be padded, the right columns may be padded)"""
    return kind in ("right", "full"), kind in ("left", "full")


def take_rows(left: pa.RecordBatch, right: pa.RecordBatch, lidx: Ids, ridx: Optional[Ids], kind: str) -> pa.RecordBatch:
    pad_l, pad_r = padded_sides(kind)
    li = pa.array(lidx, type=pa.int64())
    arrays = [c.take(li) for c in left.columns]
    fields = [f.with_nullable(True) if pad_l else f for f in left.schema]
    if ridx is not None:
        ri = pa.array(ridx, type=pa.int64())
        arrays += [c.take(ri) for c in right.columns]
        fields += [f.with_nullable(True) if pad_r else f for f in right.schema]
    return pa.RecordBatch.from_arrays(arrays, schema=pa.schema(fields))


def join(left, right, keys: Sequence[J.KeyPair], kind: str):
    """`left` / `right`: a batch or a sequence of batches -> (lidx, ridx or None, the joined batch)"""
    lb = left if isinstance(left, pa.RecordBatch) else R.join(list(left))
    rb = right if isinstance(right, pa.RecordBatch) else R.join(list(right))
    lidx, ridx = join_indices(lb, rb, keys, kind)
    return lidx, ridx, take_rows(lb, rb, lidx, ridx, kind)


def census(left, right, keys: Sequence[J.KeyPair]) -> Tuple[int, int, int]:
    """(matched left rows, unmatched left rows, unmatched right rows)"""
    lb = left if isinstance(left, pa.RecordBatch) else R.join(list(left))
    rb = right if isinstance(right, pa.RecordBatch) else R.join(list(right))
    lidx, ridx = J.join_indices(lb, rb, keys)
    return len(set(lidx)), lb.num_rows - len(set(lidx)), rb.num_rows - len(set(ridx))
