"""GPU: the SECOND round of every loop that walks its input in rounds -- the single-workgroup scans that carry a running total
from one round of tile totals into the next (scan_device.h: one loop for the join, the sort, the group heads, the string
functions and the block totals of the Parquet scan and writer, one for the count rows of partition.hip and sort.hip), and the
launches whose grid is capped so that a thread strides on to further rows (strfn.hip, like.hip, typed_ops.hip).  Each test
feeds the smallest input that puts more than one full tile (or one full wave; for Parquet, one block) into the second round,
compares the whole result with the host reference its sibling tests use, and asserts that a non-trivial part of the output is
produced by the second round.

The round sizes below restate the tiles and grid caps of the sources; tests/test_round_thresholds_host.py reads the sources
and fails when they drift apart.  Inputs are drawn from small pools of distinct values (`pool.take(indices)`), and a per-row
Python reference is evaluated once per pool entry and expanded with the same indices: the GPU work is milliseconds, the host
side is the cost.

  loop                                          one round covers          its second round is reached by
  scan_totals_in_place (scan_device.h), the shared loop over tile totals, one total per thread of one workgroup, as
    scan_totals_kernel, the join's left rows    256 tiles x 2048          test_{inner,left,semi_and_anti}_join_left_rows_past_one_scan_round
    scan_totals_kernel, FULL's right rows       256 tiles x 2048          test_full_join_tail_of_right_rows_past_one_scan_round
    scan_totals_kernel, string functions        256 tiles x 2048          test_string_functions_more_chunks_than_one_scan_round (two tiles in round
                                                                          two), and at 1 025 tiles test_gpu_strfn.py::test_more_rows_than_one_grid_pass
    sort_utf8_scan_sums_kernel, plain           256 tiles x 2048          test_sorted_utf8_payload_past_one_scan_round
    sort_utf8_scan_sums_kernel, "no row"        256 tiles x 2048          test_left_joined_utf8_payload_past_one_scan_round
    agg_head_scan_kernel                        256 tiles x 2048          every join above (the runs of the concatenated keys)
    pq_page_scan_kernel                         256 pages                 tests/parquet_forged_cases.py::more_than_256_pages
    pq_rowlen_scan_kernel (Parquet scan)        256 blocks x 4096 rows    test_parquet_scan_utf8_offsets_past_one_scan_round (PLAIN with and without
                                                                          nulls, dictionary: one block, of one row, in round two)
    pw_scan_kernel (Parquet write)              256 blocks x 4096 rows    test_parquet_write_past_one_scan_round (a batch, and a view nine rows into its
                                                                          parent: the 17th page starts at block 256)
  scan_count_rows (scan_device.h), as
    part_scan_kernel                            2048 tiles x 2048 rows    test_partition_more_tiles_than_one_scan_round (3 and 256 partitions)
  strfn_rows_kernel, strfn_gather_kernel        8192 workgroups x 256     test_string_functions_more_rows_than_one_grid_pass (wave per row in the strided
                                                                          iteration, a sliced view), ..._short_rows_in_the_strided_iteration (lane per
                                                                          row), test_gpu_strfn.py::test_more_rows_than_one_grid_pass (rows of 0..3 bytes)
  strfn_bytemap_kernel, strfn_rebase_kernel     16 MiB / 2^20 offsets     the same three (upper(s)); test_gpu_strfn.py::test_byte_map_more_bytes_...
  like_kernel                                   8192 workgroups x 256     test_like_more_rows_than_one_grid_pass (wave per row), test_like_short_rows_...,
                                                                          test_gpu_like.py::test_more_rows_than_one_grid_pass (rows of 0..3 bytes)
  cmp128_kernel, utf8_to_bool_kernel            8192 workgroups x 256     test_typed_operations_more_rows_than_one_grid_pass
  is_null_kernel                                8192 workgroups x 256     the same, and test_gpu_like.py::test_more_rows_than_one_grid_pass
  utf8_uniform_kernel                           8192 workgroups x 256     test_uniform_length_check_more_rows_than_one_grid_pass (the batch groups of
                                                                          test_gpu_scale.py take utf8_uniform_group_kernel, never this one)
  iota_offsets_kernel                           8192 workgroups x 256     the same, and test_gpu_scale.py::test_reference_schema_group_full_size (a
                                                                          joined output of some 3 x 10^7 rows, offsets compared with 8 i)
"""
import io

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

import chapterhouseqe_amd as chq
from chapterhouseqe_amd.sqlparse import parse_expr
from oracle import oracle as O

from . import join_reference as J
from . import like_reference as LR
from . import outer_join_reference as OJ
from . import partition_reference as P
from . import sort_reference as R
from . import strfn_reference as SR
from .cases import empty_aliases
from .helpers import batches_identical, explain_diff
from .test_gpu_join import aliases, int_side, same, to_host
from .test_gpu_like import POOL as LIKE_POOL
from .test_gpu_like import WAVE_MODE_BYTES as LIKE_WAVE_MODE_BYTES
from .test_gpu_parquet import check as check_scan
from .test_gpu_parity import BOOL_WORDS
from .test_gpu_sort import explain, identical, ob
from .test_gpu_strfn import POOL as STRFN_POOL
from .test_gpu_strfn import WAVE_MODE_BYTES as STRFN_WAVE_MODE_BYTES

pytestmark = pytest.mark.gpu

T = 2048                              # rows (or tile totals) per workgroup tile: kScanTile = kAggTile = kJoinTile, kPartTile, kSortTile, STRFN_SCAN_CHUNK
SCAN_ROUND = 256 * T                  # scan_totals_in_place (the join's scans, sort_utf8_scan_sums_kernel): one tile total per thread and round
PART_ROUND = T * T                    # part_scan_kernel (scan_count_rows): kPartItems tile counts per thread and round
STRFN_ROUND = 256 * T                 # scan_totals_in_place under the string functions: the same loop, the same round
STRIDE_ROWS = 8192 * 256              # rows one pass of a grid capped at 256 * 32 workgroups covers (strfn rows / gather, like, typed_ops)
BYTEMAP_BYTES = 4096 * 256 * 16       # bytes one pass of strfn_bytemap_kernel's grid covers (capped at 256 * 16 workgroups)
REBASE_ROWS = 4096 * 256              # offsets one pass of strfn_rebase_kernel's grid covers
PQ_BLOCK = 4096                       # rows per block total of the Parquet offset scan (PQ_SCAN_ROWS) and of the writer (PW_BLOCK_ROWS)
PQ_ROUND = 256 * PQ_BLOCK             # pq_rowlen_scan_kernel, pw_scan_kernel: one block total per thread and round

SCAN_ROWS = SCAN_ROUND + T + 5        # the smallest sizes that put more than one full tile into the second round
PART_ROWS = PART_ROUND + T + 5
STRFN_ROWS = STRFN_ROUND + T + 5
STRIDE_N = STRIDE_ROWS + 64 + 1       # ... more than one full wave into the strided iteration
PQ_ROWS = PQ_ROUND + 1                # ... one block total, of one row, into the second round
LONG_TAIL = 4096                      # the last rows of a strided column are long: wave-per-row mode in the strided iteration too
KK = [("k", "k")]


@pytest.fixture(scope="module")
def ctx():
    c = chq.Context(0)
    yield c
    c.close()


# ---- columns from pools ----------------------------------------------------------------------------------------------------
def utf8_pool(cells):
    """bytes / None -> a Utf8 array (None: a null slot that encloses nothing)"""
    return pa.array(cells, pa.binary()).view(pa.utf8())


def offsets_of(arr):
    return np.frombuffer(arr.buffers()[1], np.int32, len(arr) + 1, arr.offset * 4)


def byte_total(arr):
    o = offsets_of(arr)
    return int(o[-1]) - int(o[0])


def lengths_of(arr):
    return np.diff(offsets_of(arr))


def same_array(got, exp, what):
    """a computed array against the expected one, buffer by buffer: type, null count, validity, Int32 / Boolean values, or the
    offsets (from 0) and the bytes"""
    n = len(exp)
    assert got.type == exp.type and len(got) == n and got.offset == 0, (what, got.type, len(got))
    assert got.null_count == exp.null_count, (what, got.null_count, exp.null_count)
    gv, ev = np.asarray(got.is_valid()), np.asarray(exp.is_valid())
    assert np.array_equal(gv, ev), f"{what}: validity differs first at row {int(np.flatnonzero(gv != ev)[0])}"
    if pa.types.is_string(exp.type):
        go, eo = offsets_of(got), offsets_of(exp) - offsets_of(exp)[0]
        if not np.array_equal(go, eo):
            bad = np.flatnonzero(go != eo)[:4]
            raise AssertionError(f"{what}: offsets differ first at {bad.tolist()}: got {go[bad].tolist()} expected {eo[bad].tolist()}")
        total, first = int(eo[-1]), int(offsets_of(exp)[0])
        gd = np.frombuffer(got.buffers()[2], np.uint8, total) if total else np.zeros(0, np.uint8)
        ed = np.frombuffer(exp.buffers()[2], np.uint8, total, first) if total else np.zeros(0, np.uint8)
        if not np.array_equal(gd, ed):
            at = int(np.flatnonzero(gd != ed)[0])
            row = int(np.searchsorted(eo, at, side="right")) - 1
            raise AssertionError(f"{what}: byte {at} (row {row}): got {gd[at:at + 8].tobytes()!r} expected {ed[at:at + 8].tobytes()!r}")
    else:
        zero = False if pa.types.is_boolean(exp.type) else 0
        g = np.asarray(got.fill_null(zero).to_numpy(zero_copy_only=False))
        e = np.asarray(exp.fill_null(zero).to_numpy(zero_copy_only=False))
        if not np.array_equal(g[ev], e[ev]):
            bad = np.flatnonzero((g != e) & ev)[:4]
            raise AssertionError(f"{what}: values differ first at rows {bad.tolist()}: got {g[bad].tolist()} expected {e[bad].tolist()}")


# ---- joins: scan_totals_kernel over more than 256 tiles of left rows --------------------------------------------------------
def payload_strings(rng, count):
    """Utf8 payload pool: lengths 0..40 (both branches of the gather's copy: up to 32 bytes a lane, beyond that the wave), a few
    long strings, and a null"""
    cells = [bytes(rng.integers(97, 123, int(ln)).astype(np.uint8)) for ln in rng.integers(0, 41, count)]
    cells += [bytes(rng.integers(65, 91, ln).astype(np.uint8)) for ln in (33, 64, 65, 100, 300)]
    return cells + [None]


@pytest.fixture(scope="module")
def join_sides():
    """SCAN_ROWS left rows against 3 000 right rows with a Utf8 payload.  Left keys are drawn so that a good half of the rows on
    either side of row SCAN_ROUND match (two right rows on average), the rest do not, 10 % of them for a null key; left rows
    0, SCAN_ROUND - 1, SCAN_ROUND and the last one hold keys of their own, which two right rows each share"""
    rng = np.random.default_rng(20261020)
    nl, nr = SCAN_ROWS, 3000
    forced_rows, forced_keys = [0, SCAN_ROUND - 1, SCAN_ROUND, nl - 1], [10_000, 10_001, 10_002, 10_003]
    rk, rmask = rng.integers(0, 2000, nr), rng.random(nr) < 0.05
    at = rng.choice(nr, 8, replace=False)
    rk[at], rmask[at] = np.repeat(forced_keys, 2), False
    lk, lmask = rng.integers(0, 2500, nl), rng.random(nl) < 0.1
    lk[forced_rows], lmask[forced_rows] = forced_keys, False
    pool = payload_strings(rng, 200)
    s = utf8_pool(pool).take(pa.array(rng.integers(0, len(pool), nr)))
    left = int_side(lk, "lrow", lmask)
    right = pa.RecordBatch.from_arrays([pa.array(rk.astype(np.int32), mask=rmask), pa.array(np.arange(nr, dtype=np.int32)), s], names=["k", "rrow", "s"])
    assert left.num_rows > SCAN_ROUND + T                                   # more than one full tile in the scan's second round
    return left, right, forced_rows


def joined(ctx, left, right, how, device_in):
    """one join against the reference (every column, bit for bit) -> (the result on the host, the expected batch)"""
    ls = chq.DeviceRecordBatch.from_host(left, ctx) if device_in else left
    rs = chq.DeviceRecordBatch.from_host(right, ctx) if device_in else right
    got = to_host(chq.join_records(ls, aliases(left), rs, aliases(right), J.to_plan(KK), ctx=ctx, how=how))
    exp = (J.join(left, right, KK) if how == "inner" else OJ.join(left, right, KK, how))[2]
    same(got, exp)
    return got, exp


def test_inner_join_left_rows_past_one_scan_round(ctx, join_sides):
    left, right, forced = join_sides
    got, _ = joined(ctx, left, right, "inner", device_in=True)
    lrow = got.column("lrow").to_numpy()
    assert int((lrow >= SCAN_ROUND).sum()) >= 100 and int((lrow < SCAN_ROUND).sum()) >= 100
    for row in forced:                                                       # two right rows each, at both ends of both rounds
        assert int((lrow == row).sum()) == 2, row
    assert lrow[0] == 0 and lrow[-1] == left.num_rows - 1


@pytest.fixture(scope="module")
def left_joined(ctx, join_sides):
    left, right, _ = join_sides
    return joined(ctx, left, right, "left", device_in=False)


def test_left_join_left_rows_past_one_scan_round(left_joined, join_sides):
    got, _ = left_joined
    lrow = got.column("lrow").to_numpy()
    assert int((lrow >= SCAN_ROUND).sum()) >= 100
    padded = ~np.asarray(got.column("rrow").is_valid())
    assert int((padded & (lrow >= SCAN_ROUND)).sum()) >= 100 and int((~padded & (lrow >= SCAN_ROUND)).sum()) >= 100
    for row in join_sides[2]:
        assert int((lrow == row).sum()) == 2, row


@pytest.mark.parametrize("how", ["semi", "anti"])
def test_semi_and_anti_join_left_rows_past_one_scan_round(ctx, join_sides, how):
    left, right, forced = join_sides
    got, _ = joined(ctx, left, right, how, device_in=how == "semi")
    lrow = got.column("lrow").to_numpy()
    assert int((lrow >= SCAN_ROUND).sum()) >= 100 and int((lrow < SCAN_ROUND).sum()) >= 100
    assert all(int((lrow == row).sum()) == (how == "semi") for row in forced)


def test_full_join_tail_of_right_rows_past_one_scan_round(ctx):
    """FULL runs the same scan again over the flags of the RIGHT rows: SCAN_ROWS right rows, every second key on average absent
    on the left, over the whole range"""
    rng = np.random.default_rng(20261021)
    nr, nl = SCAN_ROWS, 3000
    lk, lmask = rng.permutation(nl), rng.random(nl) < 0.05
    rk, rmask = rng.integers(0, 2 * nl, nr), rng.random(nr) < 0.05
    left, right = int_side(lk, "lrow", lmask), int_side(rk, "rrow", rmask)
    assert right.num_rows > SCAN_ROUND + T
    got, _ = joined(ctx, left, right, "full", device_in=True)
    tail = ~np.asarray(got.column("lrow").is_valid())
    first = int(np.flatnonzero(tail)[0])
    assert tail[first:].all() and not tail[:first].any()                    # the tail is the end of the output
    rrow = got.column("rrow").slice(first).to_numpy()
    assert int((rrow >= SCAN_ROUND).sum()) >= 100 and int((rrow < SCAN_ROUND).sum()) >= 100
    assert (np.diff(rrow) > 0).all()                                        # in right-row order


# ---- partitioning: part_scan_kernel over more than 2048 tiles ---------------------------------------------------------------
@pytest.fixture(scope="module")
def part_rows():
    """PART_ROWS rows: an Int32 key from a pool of 1 000 values (one of them null) and the row number.  Every pool entry
    occurs among the first 1 000 rows and among the rows from PART_ROUND on; the hash of every row (the reference's, evaluated
    per pool entry and expanded) is shared by the partition counts"""
    rng = np.random.default_rng(20261022)
    n, npool = PART_ROWS, 1000
    values = (np.arange(npool, dtype=np.int64) * 4_294_311 - 2**31 + rng.integers(0, 4_000_000, npool)).astype(np.int32)   # distinct, over the whole range
    mask = np.zeros(npool, bool)
    mask[17] = True
    pool = pa.array(values, mask=mask)
    idx = rng.integers(0, npool, n)
    idx[:npool] = rng.permutation(npool)
    idx[PART_ROUND:PART_ROUND + 2 * npool] = np.arange(2 * npool) % npool
    assert n - PART_ROUND >= 2 * npool and n > PART_ROUND + T
    rec = pa.RecordBatch.from_arrays([pool.take(pa.array(idx)), pa.array(np.arange(n, dtype=np.int32))], names=["k", "row"])
    hashes = P.row_hashes(pa.RecordBatch.from_arrays([pool], names=["k"]), ["k"])[idx]
    return rec, hashes


@pytest.mark.parametrize("n_parts", [3, 256])
def test_partition_more_tiles_than_one_scan_round(ctx, part_rows, n_parts):
    rec, hashes = part_rows
    ids = P.ids_of_hashes(hashes, n_parts)
    order = np.argsort(ids, kind="stable")                                   # rows in input order inside every partition
    cuts = np.searchsorted(ids[order], np.arange(n_parts + 1))
    dev = chq.DeviceRecordBatch.from_host(rec, ctx)
    got = chq.partition_records(dev, aliases(rec), P.to_plan(["k"]), n_parts, ctx=ctx)
    assert len(got) == n_parts
    filled = 0
    for p in range(n_parts):
        g = got[p].to_host()
        same(g, rec.take(pa.array(order[cuts[p]:cuts[p + 1]])))
        if g.num_rows == 0:
            continue
        filled += 1
        rows = g.column("row").to_numpy()
        assert rows[0] < PART_ROUND <= rows[-1], p                          # rows of both rounds of the scan
        assert int((rows >= PART_ROUND).sum()) >= 2, p
        assert (np.diff(rows) > 0).all(), p
    assert filled > n_parts // 2
    s = ctx.last_stats()
    assert s["rows_in"] == rec.num_rows and s["rows_out"] == rec.num_rows and s["tiles"] > T + 1


# ---- Utf8 gather: sort_utf8_scan_sums_kernel over more than 256 output tiles ------------------------------------------------
def test_sorted_utf8_payload_past_one_scan_round(ctx):
    """(a) the plain gather: SCAN_ROWS rows ordered by a small Int16 key.  The rows of the largest key end the output; the last
    of them (output rows from SCAN_ROUND on, tiles >= 256) hold the long strings, which the wave copies together"""
    rng = np.random.default_rng(20261023)
    n = SCAN_ROWS
    k = rng.integers(0, 7, n).astype(np.int16)
    pool = payload_strings(rng, 300)
    longs = [i for i, c in enumerate(pool) if c is not None and len(c) >= 100]
    idx = rng.integers(0, len(pool), n)
    last = np.flatnonzero(k == 6)[-T:]                                       # the last T rows of key 6: output rows n - T .. n - 1
    idx[last[::97]] = np.resize(longs, len(last[::97]))
    rec = pa.RecordBatch.from_arrays([pa.array(k), utf8_pool(pool).take(pa.array(idx)), pa.array(np.arange(n, dtype=np.int32))], names=["k", "s", "row"])
    keys = [("k", False, False)]
    got = chq.sort_record(chq.DeviceRecordBatch.from_host(rec, ctx), aliases(rec), ob(keys), ctx=ctx).to_host()
    exp = R.sort_batch(rec, keys)
    assert identical(got, exp), explain(got, exp)
    assert got.num_rows > SCAN_ROUND + T
    second = lengths_of(exp.column("s"))[SCAN_ROUND:]
    assert int((second >= 100).sum()) >= 10 and int((second > 32).sum()) >= 100 and int((second <= 32).sum()) >= 100
    assert exp.column("s").slice(SCAN_ROUND).null_count > 0
    assert int(offsets_of(got.column("s"))[-1]) == byte_total(exp.column("s"))


def test_left_joined_utf8_payload_past_one_scan_round(left_joined):
    """(b) the padded gather: the right side's Utf8 payload through a LEFT join of more than SCAN_ROUND output rows, "no row"
    on both sides of output row SCAN_ROUND"""
    got, exp = left_joined
    assert got.num_rows > SCAN_ROUND + T
    padded = ~np.asarray(exp.column("rrow").is_valid())
    assert int(padded[:SCAN_ROUND].sum()) >= 100 and int(padded[SCAN_ROUND:].sum()) >= 100
    second = lengths_of(exp.column("s"))[SCAN_ROUND:]
    assert int((second > 32).sum()) >= 100 and int(((second > 0) & (second <= 32)).sum()) >= 100
    same_array(got.column("s"), exp.column("s"), "s")
    assert int(offsets_of(got.column("s"))[-1]) == byte_total(exp.column("s"))


# ---- string functions ----------------------------------------------------------------------------------------------------------
def expanded(pool_values, idx, typ):
    """what a per-row reference gives for every pool entry -> the expected column"""
    return pa.array(pool_values, typ).take(pa.array(idx)) if typ != pa.utf8() else utf8_pool(pool_values).take(pa.array(idx))


def over_pool(fn, pool, *args):
    return [None if c is None else fn(c, *args) for c in pool]


def strfn_forms(pool):
    return {
        "substring(s from 2 for 3)": (over_pool(SR.substring, pool, 2, 3), pa.utf8()),
        "trim(s)": (over_pool(SR.trim, pool), pa.utf8()),
        "rtrim(s)": (over_pool(SR.rtrim, pool), pa.utf8()),
        "s || '-' || s": (over_pool(lambda c: c + b"-" + c, pool), pa.utf8()),
        "upper(s)": (over_pool(SR.upper, pool), pa.utf8()),
        "length(s)": (over_pool(SR.length, pool), pa.int32()),
    }


def check_strfn(ctx, dev, idx, pool, sqls, what):
    forms = strfn_forms(pool)
    for sql in sqls:
        values, typ = forms[sql]
        got, is_scalar = chq.compute_value(dev, [[]], parse_expr(sql), ctx=ctx)
        assert not is_scalar, sql
        exp = expanded(values, idx, typ)
        same_array(got, exp, f"{what}: {sql}")
        if typ == pa.utf8():
            assert int(offsets_of(got)[-1]) == byte_total(exp), sql


def test_string_functions_more_chunks_than_one_scan_round(ctx):
    """scan_totals_kernel under the string functions: 258 tile totals, two of them (one full tile and five rows) behind the first
    round of 256"""
    rng = np.random.default_rng(20261024)
    n = STRFN_ROWS
    pool = list(STRFN_POOL) + [b"  two  words  ", b"\xc3\xa9\xc3\xa9\xc3\xa9\xc3\xa9", None]
    idx = rng.integers(0, len(pool), n)
    idx[STRFN_ROUND - 1], idx[STRFN_ROUND], idx[n - 1] = 6, 7, 13
    s = utf8_pool(pool).take(pa.array(idx))
    assert n > STRFN_ROUND + T and s.null_count > 0 and s.slice(STRFN_ROUND).null_count > 0
    assert int(lengths_of(s)[STRFN_ROUND:].sum()) > 0
    dev = chq.DeviceRecordBatch.from_host(pa.RecordBatch.from_arrays([s], names=["s"]), ctx)
    check_strfn(ctx, dev, idx, pool, ["substring(s from 2 for 3)", "trim(s)", "s || '-' || s"], f"{n} rows")


def strided_indices(rng, n, n_short, n_pool):
    """pool entries [0, n_short) for the bulk, [n_short, n_pool) (the long ones and the null) mixed into the last LONG_TAIL rows"""
    idx = rng.integers(0, n_short, n)
    idx[rng.random(n) < 0.1] = n_pool - 1                                    # nulls everywhere
    tail = rng.integers(n_short, n_pool, LONG_TAIL)
    idx[n - LONG_TAIL:] = tail
    return idx


def test_string_functions_more_rows_than_one_grid_pass(ctx):
    """strfn_rows_kernel and strfn_gather_kernel past 8192 workgroups, strfn_bytemap_kernel past 16 MiB, strfn_rebase_kernel past
    2^20 offsets: 9-byte rows, and about 100 bytes in each of the last 4 096 rows, so that the waves of the strided iteration
    run in both modes.  The column is a device view three rows into its parent: the offsets that are rebased do not start at 0"""
    rng = np.random.default_rng(20261025)
    n, lead = STRIDE_N, 3
    units = [b"a", b"B", b" ", b"\xc3\xa9", b"z", b"Q", b"\xe6\x97\xa5"]

    def row(length, trailing):
        out = b""
        while len(out) < length - trailing:
            u = units[int(rng.integers(0, len(units)))]
            out += u if len(out) + len(u) <= length - trailing else b"x" * (length - trailing - len(out))
        return out + b" " * trailing
    short = [row(9, int(t)) for t in rng.integers(0, 4, 200)]
    long_ = [row(int(ln), int(t)) for ln, t in zip(rng.integers(90, 111, 40), rng.integers(0, 70, 40))]
    pool = short + long_ + [None]
    idx = strided_indices(rng, n + lead, len(short), len(pool))
    idx[lead + STRIDE_ROWS], idx[lead + STRIDE_ROWS - 1] = 0, 1              # (valid rows at the seam)
    s = utf8_pool(pool).take(pa.array(idx))
    view = s.slice(lead)
    lens = lengths_of(view)
    assert len(view) > STRIDE_ROWS + 64 and byte_total(view) > BYTEMAP_BYTES + 4096 and len(view) > REBASE_ROWS + 256
    assert offsets_of(view)[0] != 0 and view.slice(STRIDE_ROWS).null_count > 0
    for w in range(STRIDE_ROWS, n - 63, 64):                                 # every wave of the strided iteration is in wave mode ...
        assert int(lens[w:w + 64].sum()) > STRFN_WAVE_MODE_BYTES, w
    assert int(lens[STRIDE_ROWS - 64 * 1024:STRIDE_ROWS - LONG_TAIL].max()) == 9   # ... and the first pass ran the lane mode too
    dev = chq.DeviceRecordBatch.from_host(pa.RecordBatch.from_arrays([s], names=["s"]), ctx).slice(lead, n)
    check_strfn(ctx, dev, idx[lead:], pool, ["upper(s)", "length(s)", "substring(s from 2 for 3)", "rtrim(s)", "s || '-' || s"], f"{n} rows")


def test_string_functions_short_rows_in_the_strided_iteration(ctx):
    """the same kernels with 9-byte rows to the end: the lane-per-row mode in the strided iteration"""
    rng = np.random.default_rng(20261026)
    n = STRIDE_N
    pool = [bytes(rng.choice(np.frombuffer(b"aB c\xc3\xa9", np.uint8)[:4], 9).astype(np.uint8)) for _ in range(60)] + [None]
    idx = rng.integers(0, len(pool), n)
    idx[STRIDE_ROWS:] = np.arange(n - STRIDE_ROWS) % len(pool)               # (every pool entry, the null too, in the strided iteration)
    s = utf8_pool(pool).take(pa.array(idx))
    assert len(pool) <= n - STRIDE_ROWS
    assert byte_total(s) > BYTEMAP_BYTES and s.slice(STRIDE_ROWS).null_count > 0 and int(lengths_of(s)[STRIDE_ROWS:].sum()) > 0
    dev = chq.DeviceRecordBatch.from_host(pa.RecordBatch.from_arrays([s], names=["s"]), ctx)
    check_strfn(ctx, dev, idx, pool, ["upper(s)", "length(s)", "substring(s from 2 for 3)", "rtrim(s)", "s || '-' || s"], f"{n} short rows")


# ---- LIKE ----------------------------------------------------------------------------------------------------------------------
def test_like_more_rows_than_one_grid_pass(ctx):
    """like_kernel past 8192 workgroups: short strings in lane-per-row mode, the last 4 096 rows about 100 bytes long, so that
    the strided iteration runs the wave-per-row mode as well; nulls in both"""
    rng = np.random.default_rng(20261027)
    n = STRIDE_N
    short = [v for v in LIKE_POOL if len(v.encode()) <= 20]
    x = "x"
    long_ = [x * 90 + "ab" + x * 8 + "c", x * 95 + "abc", "ab" + x * 100, "a" + x * 99 + "c", "abc" + x * 97, "aéc" + x * 96, x * 63 + "ab" + x * 40 + "c",
             x * 64 + "ab" + x * 30 + "cx", "axc" + x * 61 + "abc", "é" * 45 + "abzc", "ab" * 50 + "c", "ab" * 50, x * 100, "a_c%" + x * 96 + "ab%c"]
    pool = short + long_ + [None]
    idx = strided_indices(rng, n, len(short), len(pool))
    idx[STRIDE_ROWS], idx[STRIDE_ROWS - 1] = len(short), len(short) + 1
    s = pa.array(pool, pa.utf8()).take(pa.array(idx))
    lens = lengths_of(s)
    assert len(s) > STRIDE_ROWS + 64 and s.slice(STRIDE_ROWS).null_count > 0
    assert int(lens[n - LONG_TAIL:STRIDE_ROWS].sum()) > 0
    for w in range((n - LONG_TAIL + 63) & ~63, n - 63, 64):                  # whole waves of the long tail: before and behind the seam
        assert int(lens[w:w + 64].sum()) > LIKE_WAVE_MODE_BYTES, w
    assert int(lens[:n - LONG_TAIL].max()) <= 20
    dev = chq.DeviceRecordBatch.from_host(pa.RecordBatch.from_arrays([s], names=["s"]), ctx)
    for pattern, negated in (("%ab%c", False), ("a_c%", True)):
        values = LR.like_values(pool, pattern, None, negated)
        assert {True, False} <= set(values[:len(short)]) and {True, False} <= set(values[len(short):-1]), pattern
        exp = pa.array(values, pa.bool_()).take(pa.array(idx))
        got, is_scalar = chq.compute_value(dev, [[]], parse_expr(LR.like_sql("s", pattern, None, negated)), ctx=ctx)
        assert not is_scalar
        same_array(got, exp, LR.like_sql("s", pattern, None, negated))
        second = exp.slice(STRIDE_ROWS)
        assert second.null_count > 0 and second.true_count > 0 and second.false_count > 0, pattern


def test_like_short_rows_in_the_strided_iteration(ctx):
    """the same launch with short strings to the end: the lane-per-row mode in the strided iteration"""
    rng = np.random.default_rng(20261028)
    n = STRIDE_N
    pool = [v for v in LIKE_POOL if len(v.encode()) <= 20] + [None]
    idx = rng.integers(0, len(pool), n)
    idx[STRIDE_ROWS:] = np.arange(n - STRIDE_ROWS) % len(pool)               # (every pool entry, the null too, in the strided iteration)
    s = pa.array(pool, pa.utf8()).take(pa.array(idx))
    assert len(pool) <= n - STRIDE_ROWS
    dev = chq.DeviceRecordBatch.from_host(pa.RecordBatch.from_arrays([s], names=["s"]), ctx)
    for pattern, negated in (("%ab%c", False), ("a_c%", True)):
        exp = pa.array(LR.like_values(pool, pattern, None, negated), pa.bool_()).take(pa.array(idx))
        got, _ = chq.compute_value(dev, [[]], parse_expr(LR.like_sql("s", pattern, None, negated)), ctx=ctx)
        same_array(got, exp, LR.like_sql("s", pattern, None, negated))
        second = exp.slice(STRIDE_ROWS)
        assert second.null_count > 0 and second.true_count > 0 and second.false_count > 0, pattern


# ---- typed operations: cmp128_kernel, utf8_to_bool_kernel, is_null_kernel past 8192 workgroups -------------------------------
def decimal_column(lo, hi, valid=None):
    """Decimal128(30, 2) from the two 64-bit words of every value"""
    n = len(lo)
    words = np.empty((n, 2), np.uint64)
    words[:, 0], words[:, 1] = lo, hi.view(np.uint64)
    bitmap = None if valid is None else pa.py_buffer(np.packbits(valid, bitorder="little").tobytes())
    return pa.Array.from_buffers(pa.decimal128(30, 2), n, [bitmap, pa.py_buffer(words.tobytes())], null_count=0 if valid is None else int((~valid).sum()))


@pytest.fixture(scope="module")
def typed_rows():
    """x1 (with nulls), x2: Decimal128 whose high words come from seven values; a quarter of the pairs are equal, a quarter have
    equal high words and low words that differ in bit 63 (an unsigned compare of the low word decides), the rest are independent"""
    rng = np.random.default_rng(20261029)
    n = STRIDE_N
    hi1 = rng.integers(-3, 4, n).astype(np.int64)
    lo1 = rng.integers(0, 2**64, n, dtype=np.uint64)
    kind = rng.random(n)
    hi2 = np.where(kind < 0.5, hi1, rng.integers(-3, 4, n)).astype(np.int64)
    lo2 = np.where(kind < 0.25, lo1, np.where(kind < 0.5, lo1 ^ np.uint64(1 << 63), rng.integers(0, 2**64, n, dtype=np.uint64)))
    words = pa.array(BOOL_WORDS + [None], pa.utf8())
    strings = pa.array(["", "a", "null", None], pa.utf8())
    rec = pa.RecordBatch.from_arrays(
        [decimal_column(lo1, hi1, rng.random(n) >= 0.1), decimal_column(lo2, hi2),
         words.take(pa.array(rng.integers(0, len(words), n))), pa.array(rng.random(n) < 0.5, mask=rng.random(n) < 0.2),
         strings.take(pa.array(rng.integers(0, len(strings), n)))], names=["x1", "x2", "w", "flag", "s"])
    flips = (kind >= 0.25) & (kind < 0.5)
    assert int(flips[STRIDE_ROWS:].sum()) >= 8 and int((kind[STRIDE_ROWS:] < 0.25).sum()) >= 8
    assert all(rec.column(c).slice(STRIDE_ROWS).null_count > 0 for c in ("x1", "w", "flag", "s"))
    return rec


@pytest.fixture(scope="module")
def typed_device_rows(ctx, typed_rows):
    return chq.DeviceRecordBatch.from_host(typed_rows, ctx)


@pytest.mark.parametrize("sql", ["x1 < x2", "x1 = x2", "w and flag", "s is null", "s is not null"])
def test_typed_operations_more_rows_than_one_grid_pass(ctx, typed_rows, typed_device_rows, sql):
    rec = typed_rows
    assert rec.num_rows > STRIDE_ROWS + 64
    al = empty_aliases(rec)
    e = parse_expr(sql)
    # (the oracle has no IS [NOT] NULL: those two are checked against tests/like_reference.py, as in test_gpu_like.py)
    exp = LR.is_null_array(rec.column("s"), negated="not" in sql) if " is " in sql else O.compute_value(rec, al, e)[0]
    got, is_scalar = chq.compute_value(typed_device_rows, al, e, ctx=ctx)
    assert not is_scalar, sql
    same_array(got, exp, sql)
    second = exp.slice(STRIDE_ROWS)                                          # the strided iteration gives both answers (and nulls)
    assert second.true_count >= 8 and second.false_count >= 8 and (second.null_count > 0) == (" is " not in sql), sql


# ---- the uniform-length Utf8 detour of filter_record: utf8_uniform_kernel and iota_offsets_kernel past 8192 workgroups --------
@pytest.mark.parametrize("ragged_row", [None, STRIDE_ROWS + 64, STRIDE_ROWS - 1])
def test_uniform_length_check_more_rows_than_one_grid_pass(ragged_row):
    """an 8-byte Utf8 column of STRIDE_ROWS + 65 rows through a filter that keeps all but one row: the check of the offsets and
    the offsets 0, 8, 16, ... of the result both stride past one pass of their grid.  With one 7-byte value, which only the
    strided iteration of the check (or only its first pass) sees, the column must keep the ordinary string path"""
    n = STRIDE_N
    c = chq.Context(0)
    c.set_option("uniform_utf8_rows", 1000)
    lens = np.full(n, 8, np.int64)
    if ragged_row is not None:
        lens[ragged_row] = 7
    offs = np.zeros(n + 1, np.int32)
    np.cumsum(lens, out=offs[1:])
    data = (np.arange(int(offs[-1]), dtype=np.int64) * 7 % 26 + 97).astype(np.uint8)
    s = pa.Array.from_buffers(pa.utf8(), n, [None, pa.py_buffer(offs.tobytes()), pa.py_buffer(data.tobytes())], null_count=0)
    rec = pa.RecordBatch.from_arrays([pa.array(np.arange(n, dtype=np.int32)), s], names=["id", "s"])
    al = empty_aliases(rec)
    e = parse_expr("id <> 5")
    dev = chq.DeviceRecordBatch.from_host(rec, c)
    got = chq.filter_record(dev, al, e, ctx=c)
    launches = c.last_stats()["launches"]
    got = got.to_host()
    chq.filter_record(chq.DeviceRecordBatch.from_host(rec.select([0]), c), al[:1], e, ctx=c)
    bare_launches = c.last_stats()["launches"]
    c.set_option("uniform_utf8_rows", 0)
    chq.filter_record(dev, al, e, ctx=c)
    plain_launches = c.last_stats()["launches"]
    c.close()
    exp = O.filter_record(rec, al, e)
    assert exp.num_rows == n - 1 > STRIDE_ROWS + 63
    assert got.schema == exp.schema and [f.nullable for f in got.schema] == [f.nullable for f in exp.schema]
    same_array(got.column("id"), exp.column("id"), "id")
    same_array(got.column("s"), exp.column("s"), "s")
    assert int(offsets_of(got.column("s"))[-1]) == 8 * (n - 1) - (ragged_row is not None)
    if ragged_row is None:   # the check and the offsets kernel around the launches of the batch without its string column
        assert launches - bare_launches == 2, (launches, bare_launches)
    else:                    # refused: no launch more than with the rewrite switched off
        assert launches == plain_launches, (launches, plain_launches)


# ---- Parquet: the block totals of the Utf8 offset scan and of the page encoder past 256 blocks of 4096 rows ------------------
PQ_POOL = [b"", b"a", b"\xc3\xa9", b"bcd", b"a string of more than sixteen bytes", b"xy", None]


def parquet_pool_indices(rng, n):
    """pool entries for n rows: the last two rows are valid and not empty, and so are the rows on either side of every multiple
    of PQ_ROUND"""
    idx = rng.integers(0, len(PQ_POOL), n)
    idx[n - 2], idx[n - 1] = 4, 2
    for seam in range(PQ_ROUND, n, PQ_ROUND):
        idx[seam - 1] = 3
    return idx


def test_parquet_scan_utf8_offsets_past_one_scan_round(ctx):
    """pq_rowlen_sums / _scan / _offsets over 257 blocks: (a) PLAIN with nulls, (b) the same rows without nulls (no row -> value
    map), (c) a dictionary with nulls, in ONE row group (pyarrow's default would cut the table at row 2^20, one row short of
    the second round).  offsets[PQ_ROUND] and offsets[PQ_ROWS] are the two values that only the second round produces"""
    rng = np.random.default_rng(20261030)
    n = PQ_ROWS
    idx = parquet_pool_indices(rng, n)
    a = utf8_pool(PQ_POOL).take(pa.array(idx))
    b = utf8_pool([c or b"" for c in PQ_POOL]).take(pa.array(idx))
    c = utf8_pool(PQ_POOL).take(pa.array(np.concatenate([rng.permutation(idx[:n - 2]), [1, 4]])))
    assert a.null_count > 0 and b.null_count == 0 and c.null_count > 0
    table = pa.Table.from_arrays([a, b, c], schema=pa.schema([pa.field("a", pa.utf8()), pa.field("b", pa.utf8(), nullable=False), pa.field("c", pa.utf8())]))
    sink = io.BytesIO()
    pq.write_table(table, sink, compression="none", row_group_size=1 << 21, use_dictionary=["c"])
    raw = sink.getvalue()
    md = pq.ParquetFile(io.BytesIO(raw)).metadata
    assert md.num_row_groups == 1 and md.num_rows == n
    encodings = [set(md.row_group(0).column(i).encodings) for i in range(3)]
    assert "RLE_DICTIONARY" not in encodings[0] | encodings[1] and "PLAIN_DICTIONARY" not in encodings[0] | encodings[1]
    assert {"RLE_DICTIONARY", "PLAIN_DICTIONARY"} & encodings[2]
    check_scan(raw, ctx)                                                     # every column, whole, against pyarrow's reading
    f = chq.ParquetFile(raw)
    got = f.read_row_group(0, ctx=ctx).to_host()
    f.close()
    for name, col in zip("abc", (a, b, c)):
        go, eo = offsets_of(got.column(name)), offsets_of(col)
        assert len(go) == n + 1 and eo[0] == 0
        assert int(go[PQ_ROUND]) == int(eo[PQ_ROUND]) > 0, name            # the base of block 256: the carry of the first round
        assert int(go[n]) == byte_total(col) > int(go[PQ_ROUND]), name     # the grand total behind the second round


@pytest.mark.parametrize("lead", [0, 9])
def test_parquet_write_past_one_scan_round(ctx, lead):
    """pw_counts / pw_scan / pw_encode over 257 blocks: nullable Int32 (30 % nulls), Utf8 and Boolean columns of a device batch
    through record_to_parquet with the default 65 536 rows per page.  Page 16 starts at block 256: its base in the value stream
    is the first total of the scan's second round.  lead = 9: a view nine rows into its parent, validity at bit offset 9 % 8"""
    rng = np.random.default_rng(20261031 + lead)
    n = PQ_ROWS
    rows = n + lead
    valid = rng.random(rows) >= 0.3
    valid[rows - 2:] = True
    parent = pa.RecordBatch.from_arrays(
        [pa.array(rng.integers(-2**31, 2**31, rows).astype(np.int32), mask=~valid),
         utf8_pool(PQ_POOL).take(pa.array(parquet_pool_indices(rng, rows))),
         pa.array(rng.random(rows) < 0.5, mask=rng.random(rows) < 0.2)], names=["i", "s", "flag"])
    want = parent.slice(lead, n)
    assert all(want.column(k).null_count > 0 for k in range(3))
    assert all(want.column(k).slice(n - 2).null_count == 0 for k in (0, 1))
    dev = chq.DeviceRecordBatch.from_host(parent, ctx)
    raw = chq.record_to_parquet(dev.slice(lead, n) if lead else dev, ctx=ctx)
    back = pq.ParquetFile(io.BytesIO(raw))
    md = back.metadata
    assert md.num_row_groups == 1 and md.num_rows == n
    got = back.read_row_group(0).combine_chunks().to_batches()
    assert len(got) == 1 and batches_identical(got[0], want), explain_diff(got[0], want)
    for name in ("i", "s"):                                                  # page 16 is the last row alone: valid, not empty
        assert got[0].column(name)[n - 1].as_py() == want.column(name)[n - 1].as_py() not in (None, ""), name
