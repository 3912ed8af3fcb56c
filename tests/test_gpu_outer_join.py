"""GPU: the join kinds LEFT, RIGHT, FULL, LEFT_SEMI and LEFT_ANTI (chq_join_records_kind) compared exactly -- row order, NaN
payloads, nullability and null counts included -- with the host reference of tests/outer_join_reference.py (itself pinned
by tests/test_outer_join_host.py)."""
import numpy as np
import pyarrow as pa
import pytest

import chapterhouseqe_amd as chq
from chapterhouseqe_amd import sqlast as A

from . import join_reference as J
from . import outer_join_reference as OJ
from . import partition_reference as P
from .helpers import arrays_identical
from .test_gpu_join import aliases, int_side, pooled_side, same, to_host
from .test_gpu_sort import KINDS, key_array, payload_batch

pytestmark = pytest.mark.gpu

T = 2048   # sorted positions, left rows, right rows and output rows per workgroup tile (join_device.h kJoinTile)
SIZES = [0, 1, 65, T - 1, T, T + 1, 3 * T + 5]
HOWS = OJ.KINDS
NEW = [h for h in HOWS if h != "inner"]
KK = [("k", "k")]


@pytest.fixture(scope="module")
def ctx():
    return chq.Context(0)


def check(ctx, left, right, keys, how, device_in=False, device_result=None):
    """one join of two host batches (or two lists of them) against the reference; returns the result (on the host)"""
    ll = [left] if isinstance(left, pa.RecordBatch) else list(left)
    rl = [right] if isinstance(right, pa.RecordBatch) else list(right)
    ls = [chq.DeviceRecordBatch.from_host(b, ctx) for b in ll] if device_in else ll
    rs = [chq.DeviceRecordBatch.from_host(b, ctx) for b in rl] if device_in else rl
    got = chq.join_records(ls, aliases(ll[0]), rs, aliases(rl[0]), J.to_plan(keys), ctx=ctx, device_result=device_result, how=how)
    assert isinstance(got, chq.DeviceRecordBatch) == (device_in if device_result is None else device_result)
    got = to_host(got)
    same(got, OJ.join(ll, rl, keys, how)[2])
    return got


def check_all(ctx, left, right, keys, hows=HOWS, device_in=False):
    return {how: check(ctx, left, right, keys, how, device_in=device_in) for how in hows}


# ---- row counts ---------------------------------------------------------------------------------------------------------------
def sized_sides(nl, nr):
    """the two sides of test_row_counts (seeds fixed so that, from 65 rows a side on, matched left rows, unmatched left rows
    and unmatched right rows all occur: checked below against the reference alone)"""
    rng = np.random.default_rng(1000 * nl + nr)
    pool = max(nl, nr) // 2
    return pooled_side(rng, nl, pool, "lrow"), pooled_side(rng, nr, pool, "rrow")


@pytest.mark.parametrize("nl", SIZES)
def test_row_counts(ctx, nl):
    for nr in SIZES:
        left, right = sized_sides(nl, nr)
        if nl >= 65 and nr >= 65:
            assert min(OJ.census(left, right, KK)) > 0, (nl, nr)                 # (no case passes vacuously)
        for how in HOWS:
            got = check(ctx, left, right, KK, how, device_in=(nl + nr + len(how)) % 2 == 1)
            s = ctx.last_stats()
            assert s["rows_in"] == nl + nr and s["rows_out"] == got.num_rows, (how, nl, nr)


# ---- degenerate shapes ----------------------------------------------------------------------------------------------------------
def test_all_left_rows_matched_left_is_inner_but_for_nullability(ctx):
    rng = np.random.default_rng(1)
    n = 3 * T + 5
    left, right = int_side(rng.integers(0, 500, n), "lrow"), int_side(np.concatenate([np.arange(500), rng.integers(0, 500, 300)]), "rrow")
    got = check_all(ctx, left, right, KK, ["inner", "left", "semi", "anti", "full"])
    inner, lj = got["inner"], got["left"]
    assert lj.num_rows == inner.num_rows > n and got["semi"].num_rows == n and got["anti"].num_rows == 0
    assert got["full"].num_rows == inner.num_rows                                # every right key occurs on the left
    for i in range(4):
        assert arrays_identical(lj.column(i), inner.column(i)) and lj.column(i).null_count == 0
        assert lj.schema.field(i).nullable == (True if i >= 2 else inner.schema.field(i).nullable)


def test_no_row_matched(ctx):
    n = T + 7
    left, right = int_side(np.arange(n), "lrow"), int_side(np.arange(n, 2 * n + 3), "rrow")
    got = check_all(ctx, left, right, KK, device_in=True)
    assert got["inner"].num_rows == 0 and got["semi"].num_rows == 0
    assert got["left"].num_rows == n and got["anti"].num_rows == n and got["right"].num_rows == n + 3
    assert got["full"].num_rows == 2 * n + 3
    assert got["left"].column(2).null_count == n and got["full"].column(0).null_count == n + 3


def test_all_keys_null_on_one_side(ctx):
    rng = np.random.default_rng(2)
    n = T + 7
    full = pooled_side(rng, n, 50, "row")
    nulls = pa.RecordBatch.from_arrays([pa.array([None] * n, type=pa.int32()), full.column(1)], names=["k", "row"])
    for left, right in ((nulls, full), (full, nulls), (nulls, nulls)):
        got = check_all(ctx, left, right, KK)
        assert got["inner"].num_rows == 0 and got["anti"].num_rows == n and got["full"].num_rows == 2 * n   # a null matches nothing


@pytest.mark.parametrize("how", HOWS)
def test_one_side_empty(ctx, how):
    rng = np.random.default_rng(3)
    left, right = payload_batch(rng, 300), payload_batch(rng, 200)
    for l, r, rows in ((left, right.slice(0, 0), {"left": 300, "full": 300, "anti": 300}),
                       (left.slice(0, 0), right, {"right": 200, "full": 200}),
                       (left.slice(0, 0), right.slice(0, 0), {})):
        for device_in in (False, True):
            got = check(ctx, l, r, KK, how, device_in=device_in)
            assert got.num_rows == rows.get(how, 0)
            assert got.num_columns == (left.num_columns if how in ("semi", "anti") else left.num_columns + right.num_columns)


# ---- tile edges -------------------------------------------------------------------------------------------------------------------
def test_unmatched_left_rows_at_row_0_and_at_the_last_row(ctx):
    n = 3 * T + 5
    keys = np.full(n, 5)
    keys[0], keys[-1] = 1000, 1001
    got = check_all(ctx, int_side(keys, "lrow"), int_side([5, 6, 5], "rrow"), KK)
    assert got["left"].num_rows == 2 * (n - 2) + 2 and got["anti"].column(1).to_pylist() == [0, n - 1]
    assert got["left"].column(3).to_pylist()[:3] == [None, 0, 2] and got["left"].column(3).to_pylist()[-1] is None


def test_a_stretch_of_unmatched_left_rows_crosses_an_output_tile(ctx):
    left = int_side([1] + list(range(100, 100 + T + 1)) + [1], "lrow")
    right = int_side([1, 9, 1, 1], "rrow")
    got = check_all(ctx, left, right, KK)
    assert got["left"].num_rows == 3 + (T + 1) + 3 and got["left"].column(3).null_count == T + 1
    assert got["semi"].column(1).to_pylist() == [0, T + 2] and got["anti"].num_rows == T + 1
    assert got["full"].num_rows == got["left"].num_rows + 1


@pytest.mark.parametrize("tail", [T - 1, T, T + 1, 2 * T])
def test_full_tail_lengths(ctx, tail):
    """`tail` unmatched right rows spread between matched ones: the tail's offsets cross the tiles of the right rows"""
    rng = np.random.default_rng(tail)
    rkeys = np.concatenate([np.arange(10_000, 10_000 + tail), rng.integers(0, 50, 700)])
    rng.shuffle(rkeys)
    left, right = int_side(np.concatenate([np.arange(50), [77, 78]]), "lrow"), int_side(rkeys, "rrow")
    assert OJ.census(left, right, KK) == (50, 2, tail)
    got = check(ctx, left, right, KK, "full", device_in=True)
    assert got.column(0).null_count == tail and got.column(3).to_pylist()[-tail:] == sorted(np.flatnonzero(rkeys >= 10_000).tolist())
    assert check(ctx, left, right, KK, "right").num_rows == 700 + tail


def test_one_left_row_matching_many_right_rows_then_an_unmatched_one(ctx):
    n = 3 * T + 5
    left = int_side([1, 5, 2], "lrow")
    got = check_all(ctx, left, int_side(np.full(n, 5), "rrow"), KK)
    assert got["left"].num_rows == n + 2 and got["left"].column(1).to_pylist()[-1] == 2 and got["left"].column(3).to_pylist()[-1] is None
    assert got["semi"].column(1).to_pylist() == [1] and got["anti"].column(1).to_pylist() == [0, 2]
    assert got["full"].num_rows == n + 2 and got["right"].num_rows == n


@pytest.mark.parametrize("right_run", [T - 1, T, T + 1, 2 * T])
def test_split_on_a_tile_boundary_of_the_sorted_positions(ctx, right_run):
    """key 0 is the first run of the sorted positions: its right rows fill positions [0, right_run), its left rows follow"""
    left = int_side([3, 0, 1, 0, 2, 0, 1], "lrow")
    right = int_side([0] * right_run + [1, 1, 1, 4], "rrow")
    got = check_all(ctx, left, right, KK, ["left", "right", "full", "semi", "anti"], device_in=True)
    assert got["full"].num_rows == 3 * right_run + 2 * 3 + 2 + 1 and got["right"].num_rows == 3 * right_run + 2 * 3 + 1
    # ... and a run that has no left rows, ending on the boundary, in front of one that has no right rows
    left, right = int_side([1, 1, 2], "lrow"), int_side([0] * right_run + [2], "rrow")
    got = check_all(ctx, left, right, KK, ["full", "right", "left"])
    assert got["full"].num_rows == 3 + right_run and got["full"].column(0).null_count == right_run
    assert got["right"].num_rows == right_run + 1 and got["right"].column(1).null_count == right_run


# ---- padded gathers ----------------------------------------------------------------------------------------------------------------
def padded_payload(rng, n, kind, nulls, nullable, row_name):
    """an Int32 key, one payload column of `kind` (with or without nulls of its own, its field nullable or not), a row id"""
    if kind == "utf8":
        pool = ["", "a", "ab\x00", "é", "x" * 33, "y" * 64, "z" * 300, ""]
        pay = pa.array([pool[i] for i in rng.integers(0, len(pool), n)], mask=(rng.random(n) < 0.15) if nulls else None)
    else:
        pay = key_array(rng, n, kind, nulls)
    key = pa.array(rng.integers(0, max(1, n // 2), n).astype(np.int32), mask=rng.random(n) < 0.1)
    fields = [pa.field("k", pa.int32(), True), pa.field("p", pay.type, nullable or nulls), pa.field(row_name, pa.int32(), False)]
    return pa.RecordBatch.from_arrays([key, pay, pa.array(np.arange(n, dtype=np.int32))], schema=pa.schema(fields))


@pytest.mark.parametrize("kind", KINDS)
def test_every_payload_type_through_the_padded_side(ctx, kind):
    rng = np.random.default_rng(300 + KINDS.index(kind))
    for nulls, nullable in ((True, True), (False, False), (False, True)):
        left, right = padded_payload(rng, T + 300, kind, nulls, nullable, "lrow"), padded_payload(rng, T + 100, kind, nulls, nullable, "rrow")
        assert min(OJ.census(left, right, KK)) > 0
        got = check(ctx, left, right, KK, "full", device_in=kind in ("float32", "utf8", "decimal", "bool"))
        assert all(f.nullable for f in got.schema)                            # non-nullable input fields come out nullable
        lpad, rpad = OJ.census(left, right, KK)[2], OJ.census(left, right, KK)[1]
        if not nulls:
            assert got.column(1).null_count == lpad and got.column(4).null_count == rpad     # exactly the padding
        lj = check(ctx, left, right, KK, "left")
        assert [f.nullable for f in lj.schema] == [f.nullable for f in left.schema] + [True] * 3
        check(ctx, left, right, KK, "right", device_in=True)


@pytest.mark.parametrize("kind", ["decimal", "decimal32", "decimal64", "decimal128_edges"])
def test_every_key_type_of_the_decimals(ctx, kind):
    """decimal keys of 4, 8 and 16 bytes through every join kind: both sides draw from one pool (nulls among them), so matched
    rows, unmatched rows and null keys all occur"""
    rng = np.random.default_rng(400 + KINDS.index(kind))
    pool = key_array(rng, 300, kind, True)
    sides = [pa.RecordBatch.from_arrays([pool.take(pa.array(rng.integers(0, 300, n))), pa.array(np.arange(n, dtype=np.int32))], names=["k", row])
             for n, row in ((1500, "lrow"), (1000, "rrow"))]
    assert min(OJ.census(*sides, KK)) > 0
    got = check_all(ctx, *sides, KK, device_in=kind == "decimal64")
    assert got["full"].num_rows > got["left"].num_rows > got["inner"].num_rows > 0 and got["anti"].num_rows >= sides[0].column(0).null_count > 0


def test_payload_of_every_importable_type_on_both_sides(ctx):
    rng = np.random.default_rng(33)
    left, right = payload_batch(rng, 700), payload_batch(rng, 600)
    for keys in ([("k", "k"), ("u8", "u8")], [("u8", "u8")], [("s", "s")]):
        assert min(OJ.census(left, right, keys)) > 0
        check_all(ctx, left, right, keys, NEW, device_in=len(keys) == 2)
    check_all(ctx, left, right, KK, NEW)                                      # every row of both sides matched


@pytest.mark.parametrize("offset,length", [(1, 3000), (9, 2049), (13, 0)])
def test_sliced_device_views(ctx, offset, length):
    rng = np.random.default_rng(offset)
    lp, rp = payload_batch(rng, 4000), payload_batch(rng, 400)
    lv = chq.DeviceRecordBatch.from_host(lp, ctx).slice(offset, length)
    rv = chq.DeviceRecordBatch.from_host(rp, ctx).slice(7, 300)
    for how in NEW:
        for keys in ([("s", "s"), ("u8", "u8")], [("b", "b"), ("k", "k")]):
            got = chq.join_records(lv, aliases(lp), rv, aliases(rp), J.to_plan(keys), ctx=ctx, how=how).to_host()
            same(got, OJ.join(lp.slice(offset, length), rp.slice(7, 300), keys, how)[2])
    got = chq.join_records(lp.slice(offset, length), aliases(lp), rp.slice(7, 300), aliases(rp), J.to_plan([("s", "s")]), ctx=ctx, how="full")
    same(got, OJ.join(lp.slice(offset, length), rp.slice(7, 300), [("s", "s")], "full")[2])


def test_groups_of_several_batches_with_empty_batches_and_mixed_residency(ctx):
    rng = np.random.default_rng(8)
    lp, rp = payload_batch(rng, 5000), payload_batch(rng, 3000)

    def windows(n):
        cuts = np.sort(rng.integers(0, n, 9)).tolist()
        cuts[4] = cuts[3]          # an empty batch
        return list(zip([0] + cuts, cuts + [n]))

    lw, rw = windows(5000), windows(3000)
    lh, rh = [lp.slice(a, b - a) for a, b in lw], [rp.slice(a, b - a) for a, b in rw]
    ld, rd = chq.DeviceRecordBatch.from_host(lp, ctx), chq.DeviceRecordBatch.from_host(rp, ctx)
    lmix = [ld.slice(a, b - a) if i % 3 else lh[i] for i, (a, b) in enumerate(lw)]
    rmix = [rh[i] if i % 2 else rd.slice(a, b - a) for i, (a, b) in enumerate(rw)]
    keys = [("u8", "u8"), ("b2", "b2")]
    assert min(OJ.census(lh, rh, keys)) > 0
    for how in NEW:
        got = chq.join_records(lmix, aliases(lp), rmix, aliases(rp), J.to_plan(keys), ctx=ctx, how=how)
        assert isinstance(got, pa.RecordBatch)          # not every input on the device: a host result
        same(got, OJ.join(lh, rh, keys, how)[2])


# ---- multiple keys ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_keys", [2, 3])
def test_several_keys_with_nulls_in_different_keys(ctx, n_keys):
    rng = np.random.default_rng(20 + n_keys)

    def side(n, row_name):
        cols = [pa.array([["x", "y", "xy", ""][i] for i in rng.integers(0, 4, n)], mask=rng.random(n) < 0.1),
                pa.array(rng.choice([0.0, -0.0, np.nan, 1.0], n).astype(np.float64), mask=rng.random(n) < 0.1),
                pa.array(rng.integers(0, 40, n).astype(np.int16), mask=rng.random(n) < 0.1)][:n_keys]
        return pa.RecordBatch.from_arrays(cols + [pa.array(np.arange(n, dtype=np.int32))], names=["s", "f", "i"][:n_keys] + [row_name])

    left, right = side(3000, "lrow"), side(300, "rrow")
    keys = [(n, n) for n in ["s", "f", "i"][:n_keys]]
    assert min(OJ.census(left, right, keys)) > 0
    check_all(ctx, left, right, keys, NEW, device_in=n_keys == 3)


def test_nine_keys_take_two_split_launches(ctx):
    rng = np.random.default_rng(22)

    def side(n, row_name):
        cols = [pa.array(rng.integers(0, 2, n).astype(np.int8), mask=(rng.random(n) < 0.05) if i in (0, 8) else None) for i in range(9)]
        return pa.RecordBatch.from_arrays(cols + [pa.array(np.arange(n, dtype=np.int32))], names=[f"k{i}" for i in range(9)] + [row_name])

    left, right = side(3000, "lrow"), side(250, "rrow")
    keys = [(f"k{i}", f"k{i}") for i in range(9)]
    m, ul, ur = OJ.census(left, right, keys)
    assert min(m, ul, ur) > 0 and ur > OJ.census(left, right, keys[:8])[2]       # the ninth key's nulls unmatch right rows
    check_all(ctx, left, right, keys, NEW)


# ---- determinism ---------------------------------------------------------------------------------------------------------------------
def raw(col):
    """the value bytes of a fixed-width column, the slots under nulls included"""
    buf = col.buffers()[1]
    w = col.type.bit_width // 8
    return buf.to_pybytes()[col.offset * w:(col.offset + len(col)) * w]


def test_two_calls_give_bit_identical_results_and_zeroed_padding(ctx):
    rng = np.random.default_rng(41)
    left, right = payload_batch(rng, 5000), payload_batch(rng, 4000)
    keys = [("u8", "u8"), ("b2", "b2")]
    assert min(OJ.census(left, right, keys)) > 0
    plan = J.to_plan(keys)
    lidx, ridx, _ = OJ.join(left, right, keys, "full")
    runs = [chq.join_records(left, aliases(left), right, aliases(right), plan, ctx=ctx, how="full", device_result=dr) for dr in (False, True, False)]
    a, b, c = [to_host(r) for r in runs]
    same(a, b)
    same(a, c)
    nl = left.num_columns
    for i, f in enumerate(a.schema):
        col, idx = a.column(i), (lidx if i < nl else ridx)
        pad = [j for j, x in enumerate(idx) if x is None]
        if pa.types.is_boolean(f.type):
            bits = np.unpackbits(np.frombuffer(col.buffers()[1], np.uint8), bitorder="little")[col.offset:col.offset + len(col)]
            assert not bits[pad].any(), f.name
            assert col.buffers()[1].to_pybytes() == b.column(i).buffers()[1].to_pybytes()
        elif pa.types.is_string(f.type):
            offs = np.frombuffer(col.buffers()[1], np.int32)[col.offset:col.offset + len(col) + 1]
            assert not np.diff(offs)[pad].any(), f.name                       # length 0 under a padded null
            assert col.buffers()[2].to_pybytes()[:offs[-1]] == b.column(i).buffers()[2].to_pybytes()[:offs[-1]]
        else:
            w = f.type.bit_width // 8
            bytes_a = np.frombuffer(raw(col), np.uint8).reshape(len(col), w)
            assert not bytes_a[pad].any(), f.name                             # zero bytes under a padded null
            assert raw(col) == raw(b.column(i)) == raw(c.column(i)), f.name


# ---- errors -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [6, -1])
def test_an_unknown_kind_through_the_c_abi(ctx, kind, monkeypatch):
    from chapterhouseqe_amd import record_utils
    monkeypatch.setitem(record_utils._JOIN_KINDS, "bogus", kind)          # past the binding's own check: the C call refuses it
    left = int_side([1, 2], "lrow")
    with pytest.raises(chq.ChqError) as ei:
        chq.join_records(left, aliases(left), left, aliases(left), J.to_plan(KK), ctx=ctx, how="bogus")
    assert ei.value.code == 22 and str(kind) in str(ei.value)


@pytest.mark.parametrize("how", NEW)
def test_errors_are_those_of_inner(ctx, how):
    rng = np.random.default_rng(3)
    left, right = payload_batch(rng, 100), payload_batch(rng, 80)
    la, ra = aliases(left), aliases(right)
    k = A.ident("k")
    cases = [([], 22), ([(k, A.ident("u8"))], 30), ([(A.ident("nope"), k)], 7), ([(k, A.ident("nope"))], 7),
             ([(A.ident("fsb16"), A.ident("fsb16"))], 30)]
    for keys, code in cases:
        codes = []
        for h in ("inner", how):
            with pytest.raises(chq.ChqError) as ei:
                chq.join_records(left, la, right, ra, keys, ctx=ctx, how=h)
            codes.append(ei.value.code)
        assert codes == [code, code], (keys, codes)


def test_right_names_the_callers_columns_in_the_callers_order(ctx):
    rng = np.random.default_rng(3)
    left, right = payload_batch(rng, 100), payload_batch(rng, 80)
    msgs = []
    for how in ("inner", "right"):
        with pytest.raises(chq.ChqError) as ei:
            chq.join_records(left, aliases(left), right, aliases(right), [(A.ident("k"), A.ident("u8"))], ctx=ctx, how=how)
        msgs.append(str(ei.value))
    assert msgs[0] == msgs[1] and msgs[1].index("'k'") < msgs[1].index("'u8'")
    with pytest.raises(chq.ChqError) as ei:          # `row` exists on both sides, `nope` on neither: the left key is the one refused
        chq.join_records(left, aliases(left), right, aliases(right), [(A.ident("nope"), A.ident("row"))], ctx=ctx, how="right")
    assert ei.value.code == 7 and "nope" in str(ei.value)


# ---- partitioned ------------------------------------------------------------------------------------------------------------------------
def rows_of(batches):
    rows = []
    for b in batches:
        rows += list(zip(*[c.to_pylist() for c in b.columns]))
    return sorted(rows, key=repr)


@pytest.mark.parametrize("how", NEW)
def test_join_partition_by_partition_is_the_whole_join(ctx, how):
    rng = np.random.default_rng(50)

    def side(n, row_name):
        return pa.RecordBatch.from_arrays([pa.array(rng.integers(0, 2000, n).astype(np.int32), mask=rng.random(n) < 0.15),
                                           pa.array(np.arange(n, dtype=np.int32))], names=["k", row_name])

    left, right = side(5000, "lrow"), side(3000, "rrow")
    assert min(OJ.census(left, right, KK)) > 0
    la, ra = aliases(left), aliases(right)
    lparts = chq.partition_records(chq.DeviceRecordBatch.from_host(left, ctx), la, P.to_plan(["k"]), 8, ctx=ctx)
    rparts = chq.partition_records(right, ra, P.to_plan(["k"]), 8, ctx=ctx, device_result=True)
    pieces = []
    for lp, rp in zip(lparts, rparts):
        got = chq.join_records(lp, la, rp, ra, J.to_plan(KK), ctx=ctx, how=how).to_host()
        same(got, OJ.join(lp.to_host(), rp.to_host(), KK, how)[2])
        pieces.append(got)
    whole = OJ.join(left, right, KK, how)[2]
    assert whole.num_rows > 1000 and sum(1 for g in pieces if g.num_rows) == 8
    assert rows_of(pieces) == rows_of([whole])
