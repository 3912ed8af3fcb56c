"""GPU: the call statistics of the operators that stand on the stable sort -- ORDER BY, GROUP BY, the window functions, JOIN
and the hash partitioning -- pinned against tests/golden/sorted_ops_stats.json.

`rows_in`, `rows_out`, `tiles`, `launches`, `bytes_read_alg` and `bytes_written_alg` of `Context.last_stats()` are the
observable trace of a call's launch sequence: a launch more or fewer, a pass over other columns or a buffer of another size
moves them.  The golden holds what the engine reported BEFORE the run finder, the aggregate typing and the end-of-call block
of the five operators were merged into one copy each, so this module says that merging them changed no call.  `kernel_ns`
is a time and is never compared.

The golden was recorded by running this module as a script (`python -m tests.test_gpu_sorted_stats OUT.json`) against a
library built from the engine sources of the commit before that change; it holds no value computed by hand.  The inputs are
plain arithmetic in the row number, so they do not depend on a random generator's version."""
import json
import os
import sys

import pyarrow as pa
import pytest

import chapterhouseqe_amd as chq
from chapterhouseqe_amd import sqlast as A

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sorted_ops_stats.json")
KEYS = ("rows_in", "rows_out", "tiles", "launches", "bytes_read_alg", "bytes_written_alg")
T = 2048                       # rows per workgroup tile of every operator here
ROWS = (0, 1, T, 3 * T + 5)    # empty, a single row, exactly one tile, several tiles with a ragged tail
BITS = [f"c{j}" for j in range(9)]   # nine keys: one more than a heads / hash launch takes (kAggMaxKeys, kPartMaxKeys)
JOIN_KINDS = ("inner", "left", "right", "full", "semi", "anti")


def batch(n, prefix=""):
    """rows 0 .. n-1 of the fixed input, the column names under `prefix`"""
    rows = range(n)
    cols = [pa.array([None if i % 11 == 0 else (i * 7919) % 13 for i in rows], type=pa.int32()),
            pa.array(["".join(chr(97 + (i * (j + 1)) % 7) for j in range(1 + i % 3)) for i in rows], type=pa.utf8()),
            pa.array([i - 1000 for i in rows], type=pa.int64()),
            pa.array([None if i % 5 == 0 else (i % 17) * 0.5 for i in rows], type=pa.float64())]
    cols += [pa.array([(i >> j) & 1 for i in rows], type=pa.int8()) for j in range(9)]
    return pa.RecordBatch.from_arrays(cols, names=[prefix + c for c in ["k1", "k2", "v", "f"] + BITS])


def thirds(rec):
    a, b = rec.num_rows // 3, 2 * rec.num_rows // 3
    return [rec.slice(0, a), rec.slice(a, b - a), rec.slice(b)]


def aliases(rec):
    return [[] for _ in range(rec.num_columns)]


def ids(names):
    return [A.ident(c) for c in names]


ORDER_BY = [A.OrderByExpr(A.ident("k1"), asc=False, nulls_first=True), A.OrderByExpr(A.ident("k2"))]
AGG_ITEMS = [A.AggItem(A.AggKind.COUNT_STAR, "n"), A.AggItem(A.AggKind.COUNT, "n_f", column=A.ident("f")),
             A.AggItem(A.AggKind.SUM, "sum_v", column=A.ident("v")), A.AggItem(A.AggKind.SUM, "sum_f", column=A.ident("f")),
             A.AggItem(A.AggKind.MIN, "min_f", column=A.ident("f")), A.AggItem(A.AggKind.MAX, "max_v", column=A.ident("v"))]
WIN_ITEMS = [A.WindowItem(A.WindowKind.ROW_NUMBER, "rn"), A.WindowItem(A.WindowKind.RANK, "rk"),
             A.WindowItem(A.WindowKind.LAG, "lag_f", A.ident("f"), offset=1),
             A.WindowItem(A.WindowKind.SUM, "sum_f", A.ident("f"), A.WindowFrame.RANGE_TO_CURRENT),
             A.WindowItem(A.WindowKind.COUNT, "n_f", A.ident("f"), A.WindowFrame.ROWS_TO_CURRENT),
             A.WindowItem(A.WindowKind.MIN, "min_v", A.ident("v"), A.WindowFrame.PARTITION)]
WIN_BARE = [A.WindowItem(A.WindowKind.COUNT_STAR, "n"), A.WindowItem(A.WindowKind.DENSE_RANK, "dr")]


def operators(ctx, n):
    """(name, call) of every pinned operator variant at n rows; call(src) takes a batch (host or device) or a list of batches"""
    rec = batch(n)
    al = aliases(rec)
    rights = {"r0": batch(0, "r_"), "r3": batch(n // 3, "r_")}
    one = {"sort": chq.sort_record, "agg": chq.aggregate_record, "win": chq.window_record}
    many = {"sort": chq.sort_records, "agg": chq.aggregate_records, "win": chq.window_records}

    def single(op, *args, **kw):   # the *_record entry for one batch, the *_records entry for a list
        return lambda src: (many if isinstance(src, list) else one)[op](src, al, *args, ctx=ctx, **kw)

    def join(right, keys, how):
        pairs = [(A.ident(k), A.ident("r_" + k)) for k in keys]
        return lambda src: chq.join_records(src, al, right, aliases(right), pairs, ctx=ctx, how=how)

    ops = [("sort/k1_desc_nulls_first,k2", single("sort", ORDER_BY)),
           ("sort/k1_desc_nulls_first,k2/limit10", single("sort", ORDER_BY, limit=10)),
           ("agg/by_k1", single("agg", ids(["k1"]), [A.AggItem(A.AggKind.KEY, "k1", key_index=0)] + AGG_ITEMS)),
           ("agg/no_key", single("agg", [], AGG_ITEMS)),
           ("agg/by_c0..c8", single("agg", ids(BITS), [A.AggItem(A.AggKind.KEY, "c8", key_index=8)] + AGG_ITEMS)),
           ("win/by_k1_order_v", single("win", ids(["k1"]), [A.OrderByExpr(A.ident("v"))], WIN_ITEMS)),
           ("win/bare", single("win", [], [], WIN_BARE))]
    for rname, right in rights.items():
        ops += [(f"join/{how}/k1/{rname}", join(right, ["k1"], how)) for how in JOIN_KINDS]
    ops += [("join/inner/c0..c8/r3", join(rights["r3"], BITS, "inner")),
            ("part/c0..c8/3", lambda src: chq.partition_records(src, al, ids(BITS), 3, ctx=ctx)),
            ("part/k2/1", lambda src: chq.partition_records(src, al, ids(["k2"]), 1, ctx=ctx))]
    return rec, ops


def measure(ctx, n):
    """{case name: the pinned counters} of every operator at n rows: on a device batch, on a host batch and on three host slices"""
    rec, ops = operators(ctx, n)
    sources = {"device": chq.DeviceRecordBatch.from_host(rec, ctx), "host": rec, "slices": thirds(rec)}
    out = {}
    for name, call in ops:
        for sname, src in sources.items():
            call(src)
            stats = ctx.last_stats()
            out[f"n{n}/{name}/{sname}"] = {k: int(stats[k]) for k in KEYS}
    return out


@pytest.fixture(scope="module")
def ctx():
    return chq.Context(0)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("n", ROWS)
def test_stats_are_the_recorded_ones(ctx, golden, n):
    got = measure(ctx, n)
    exp = {k: v for k, v in golden.items() if k.startswith(f"n{n}/")}
    assert sorted(got) == sorted(exp)
    assert len(got) == 3 * (7 + 13 + 2)
    diff = {k: (got[k], exp[k]) for k in got if got[k] != exp[k]}
    assert not diff, diff


if __name__ == "__main__":
    context = chq.Context(0)
    recorded = {}
    for rows in ROWS:
        recorded.update(measure(context, rows))
    with open(sys.argv[1], "w") as f:
        json.dump(recorded, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(recorded)} cases recorded")
