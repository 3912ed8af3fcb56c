"""GPU: what the two host fast paths of chq_filter_record take and what they refuse (filter.cpp: plain_host_columns --
every column fixed-width, not Boolean / Utf8, free of nulls).  A batch with a Boolean column, a Utf8 column or real nulls
must come back exactly as the general path returns it; a column that merely carries a validity bitmap whose nulls nobody
has counted (null_count = -1, every bit set) is still taken.  Against the oracle and against a context with both paths
switched off: same rows, same order, same null counts.  Small path: 2 rows (its lower bound) and 65 (one past a 64-row
group).  Large path: 16 384 + 1 rows in chunks of 16 384, i.e. a full chunk and a one-row tail."""
import numpy as np
import pyarrow as pa
import pytest

import chapterhouseqe_amd as chq
from chapterhouseqe_amd import record_utils
from chapterhouseqe_amd.sqlparse import parse_expr
from oracle import oracle as O

from .helpers import batches_identical, explain_diff

pytestmark = pytest.mark.gpu

REFUSED = ["bool", "utf8", "nulls", "nulls_uncounted"]
TAKEN = ["bitmap_uncounted"]
PREDICATES = ["v > 10.0", "id % 2 = 0 and v < 90.0"]


def batch(n, kind):
    rng = np.random.default_rng(n)
    cols = {"id": pa.array(np.arange(n, dtype=np.int32)), "v": pa.array((rng.random(n) * 100).astype(np.float32))}
    d = rng.random(n) * 10
    if kind == "bool":
        cols["x"] = pa.array(rng.random(n) < 0.5)
    elif kind == "utf8":
        cols["x"] = pa.array(["s%d" % (i % 7) for i in range(n)])
    elif kind in ("nulls", "nulls_uncounted"):
        mask = np.zeros(n, dtype=bool)
        mask[::3] = True
        mask[-1] = True                                   # (the one-row tail chunk of the large path holds a null)
        cols["x"] = pa.array(d, mask=mask)
    else:                                                 # a validity bitmap with every bit set
        ones = pa.py_buffer(np.full((n + 7) // 8, 0xFF, dtype=np.uint8).tobytes())
        cols["x"] = pa.Array.from_buffers(pa.float64(), n, [ones, pa.py_buffer(d.tobytes())])
    return pa.record_batch(cols)


@pytest.fixture()
def uncounted(monkeypatch):
    """Host batches reach the library the way a producer that has not counted its nulls exports them: null_count = -1 on
    every column with a validity bitmap (legal in the Arrow C Data Interface; pyarrow itself counts before it exports)."""
    export = record_utils._export_host

    def export_uncounted(rec):
        cb = export(rec)
        for i in range(cb.array.array.n_children):
            child = cb.array.array.children[i].contents
            if child.n_buffers > 0 and child.buffers[0]:
                child.null_count = -1
        return cb

    def use(kind):
        if kind.endswith("uncounted"):
            monkeypatch.setattr(record_utils, "_export_host", export_uncounted)
    return use


@pytest.fixture()
def general():
    c = chq.Context(0)
    c.set_option("small_host", 0)
    c.set_option("large_host", 0)
    yield c
    c.close()


def check(fast, general, rec, kind, launches_when_taken):
    al = chq.get_record_table_aliases(None, rec)
    for where in PREDICATES:
        e = parse_expr(where)
        exp = O.filter_record(rec, al, e)
        got = chq.filter_record(rec, al, e, ctx=fast)
        launches = fast.last_stats()["launches"]
        ref = chq.filter_record(rec, al, e, ctx=general)
        assert batches_identical(got, exp), f"{kind}, {where}:\n{explain_diff(got, exp)}"
        assert batches_identical(got, ref), f"{kind}, {where}:\n{explain_diff(got, ref)}"
        assert [c.null_count for c in got.columns] == [c.null_count for c in ref.columns] == [c.null_count for c in exp.columns]
        if kind in TAKEN:
            assert launches == launches_when_taken, (kind, where)
        else:
            assert launches == general.last_stats()["launches"], (kind, where)   # it took the general path


@pytest.mark.parametrize("kind", REFUSED + TAKEN)
@pytest.mark.parametrize("n", [2, 65])
def test_small_host_path_takes_only_plain_columns(general, uncounted, n, kind):
    uncounted(kind)
    fast = chq.Context(0)
    try:
        check(fast, general, batch(n, kind), kind, launches_when_taken=1)
    finally:
        fast.close()


@pytest.mark.parametrize("kind", REFUSED + TAKEN)
def test_large_host_path_takes_only_plain_columns(general, uncounted, kind):
    uncounted(kind)
    n = 16_384 + 1
    fast = chq.Context(0)
    fast.set_option("small_host", 0)                      # (it would take a batch of this size first)
    fast.set_option("large_host_rows", n)
    fast.set_option("large_host_chunk", 1)                # rounded up to 16 384 rows: a full chunk and a one-row tail
    try:
        check(fast, general, batch(n, kind), kind, launches_when_taken=2)   # one launch per chunk; unchunked: one
    finally:
        fast.close()


GROUP_ROWS = [2, 65, 2049]


def run_group(ctx, recs, where):
    """chq_filter_records over host batches: (outputs, launches, tiles)"""
    got = chq.filter_records(recs, chq.get_record_table_aliases(None, recs[0]), parse_expr(where), ctx=ctx)
    st = ctx.last_stats()
    print(where, [r.num_rows for r in recs], st)
    return got, st["launches"], st["tiles"]


def test_host_group_with_uncounted_all_valid_bitmaps_is_a_plain_group(uncounted):
    """every validity bit set, null_count = -1: the group scan counts, finds no null and runs the group as it runs the same
    batches without the column -- one launch over all of them, the bitmap dropped from the output as the oracle drops it"""
    uncounted("bitmap_uncounted")
    recs = [batch(n, "bitmap_uncounted") for n in GROUP_ROWS]
    bare = [r.select(["id", "v"]) for r in recs]
    c = chq.Context(0)
    try:
        for where in PREDICATES:
            al, e = chq.get_record_table_aliases(None, recs[0]), parse_expr(where)
            got, launches, tiles = run_group(c, recs, where)
            _, bare_launches, bare_tiles = run_group(c, bare, where)
            assert (launches, tiles) == (bare_launches, bare_tiles), where
            for r, g in zip(recs, got):
                exp = O.filter_record(r, al, e)
                one = chq.filter_record(r, al, e, ctx=c)
                assert batches_identical(g, exp), f"{where}:\n{explain_diff(g, exp)}"
                assert batches_identical(g, one), f"{where}:\n{explain_diff(g, one)}"
                assert [x.null_count for x in g.columns] == [x.null_count for x in exp.columns]
    finally:
        c.close()


def test_host_group_with_uncounted_nulls_in_one_batch_leaves_the_one_launch_path(uncounted):
    """the same group with real, uncounted nulls in the middle batch only: the scan must find them -- the group is joined on
    the host exactly as when the producer had counted them, and is not run as the plain group of the test above"""
    kinds = ["bitmap_uncounted", "nulls_uncounted", "bitmap_uncounted"]
    recs = [batch(n, k) for n, k in zip(GROUP_ROWS, kinds)]
    bare_recs = [r.select(["id", "v"]) for r in recs]
    c = chq.Context(0)
    try:
        counted = {where: run_group(c, recs, where)[1:] for where in PREDICATES}   # (exported by pyarrow: nulls counted)
        bare = {where: run_group(c, bare_recs, where)[1:] for where in PREDICATES}
        uncounted("nulls_uncounted")
        for where in PREDICATES:
            al, e = chq.get_record_table_aliases(None, recs[0]), parse_expr(where)
            got, launches, tiles = run_group(c, recs, where)
            assert (launches, tiles) == counted[where], where
            assert (launches, tiles) != bare[where], where
            for r, g in zip(recs, got):
                exp = O.filter_record(r, al, e)
                assert batches_identical(g, exp), f"{where}:\n{explain_diff(g, exp)}"
                assert [x.null_count for x in g.columns] == [x.null_count for x in exp.columns]
    finally:
        c.close()
