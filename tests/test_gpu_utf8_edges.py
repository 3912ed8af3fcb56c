"""GPU: Utf8 columns through filter_record and filter_records at every copy and compare threshold, against the numpy reference
of tests/utf8_reference.py (which tests/test_utf8_reference.py ties to pyarrow and the oracle on the CPU tier): output offsets,
data bytes, validity and null count from the result's buffers, and the `id` column that proves the rows.

The batch is `sel: Int32 (0 / 1), s: Utf8, id: Int32 (row number)` and the predicate `sel = 1`, so a test owns the selection
exactly; 3 x 16 384 + 101 rows: three complete tiles of the largest tile kind (24 of kinds 1 and 2) and an incomplete last group.
Every byte of `s` names its row and its place in the row (utf8_reference.make_utf8).

Which route a column takes (filter.cpp: plan_fold / follow_ups / uniform_detour) is proved, not assumed: the same call runs on
the batch without its string columns and the difference of `last_stats()["launches"]` must be
    + 0  fold, bytes inside filter_fused_kernel           fold_utf8 = 1, tile kinds 0 / 1, span <= 24 x rows, 1st / 2nd Utf8 column
    + 1  fold, offsets only, then utf8_copy_kernel        the same, span > 24 x rows
    + 1  utf8_filter_kernel                               fold_utf8 = 0 or tile kind 2 or 3rd and later column; span <= 24 x rows
    + 2  utf8_offsets_kernel, then utf8_copy_kernel       the same, span > 24 x rows
    + 2  uniform rewrite (utf8_uniform_kernel, iota_offsets_kernel): the column itself goes through the fixed-width copy
    + 1  on top, per column with nulls (bit_compact_kernel compacts its validity)
(read from filter.cpp; `split_rows` = 1 adds the tail launch to both calls alike).

Which kernel branch a cell of profile x selection reaches:
  column short (fold with bytes / utf8_filter_kernel): per 64-row group, selected bytes <= 24 x selected rows -> one lane per row:
      bytes 0..7 and 8..15 in 8- / 4-byte accesses (const 4, 8, 12, 16 sit on the `>=` of each), a 4-byte loop from byte 16
      (const 17, 23, 24; cycle41), a 1..3-byte tail (const 1, 3, 7, 11, 15, 17, 23).  Above 24 x rows -> copy_rows_wide: the long
      groups of `mixed`, the odd groups of group24 under `all` (1537 bytes of 64 rows; the even ones hold exactly 1536 and stay
      on the one-lane path), both kinds of group24 under the partial selections, the `spike` groups whatever the selection
      leaves of them (one 70 000-byte row beside empty ones, in lane 0, lane 63, mid-group; `spike4`: four in a row).
  copy_rows_wide: 16 rows per step, 8 lanes per row -- count / scatter 15, 16, 17 and 63, lane0 / lane63 / count1 (one row);
      16-byte chunks, 128 bytes per pass, then len & 15 in 4-byte and 1-byte pieces -- const 127, 128, 129, 143, 255, 257 in
      utf8_copy_kernel's scattered branch, 90..129 in `mixed`.
  column long (utf8_copy_kernel): runs x 4 > selected rows -> copy_rows_wide (alternate, runs3, scatter, lane0, random50),
      else run by run (all, runs4, runs5, count c, random98, tiles_off).  Run bytes: runs3088_all / runs3088_runs4 put 1023 ..
      8200 bytes into one run (lane 0 enters the four-chunk step at 3088 bytes, the 1 KiB step ends at nbytes & ~15, the byte
      tail is nbytes & 15); const 25 and 33 under runs4 / runs5 give runs of 100 .. 165 bytes (fewer than 64 chunks).
  tiles_off, none, first_and_last_row: tiles and groups without a selected row between selected ones (the byte scan carries).

The uniform-length rewrite, slices of device views (a first byte at an odd address), host input, nulls (bytes kept under a null
and empty), batch groups and the row counts 1 / 63 / 64 / 65 run cycle41 and const 129 (const 1 .. 16 for the rewrite) through
the same comparison.  The Utf8 comparison (strcmp_op) is checked on a table of byte strings crossed with itself -- bytes >=
0x80, embedded NULs, prefixes, a difference in the last of 300 bytes, nulls on either side -- against Python's `bytes` order.
Columns holding bytes that are not UTF-8 (80 and ff alone) are staged as they are: neither pyarrow's from_buffers nor the
library validates them, so they take part in the column-against-column forms.

Batch groups (filter_records; group_plan.cpp: plan_group, group.cpp: filter_group) are proved by `launches` and `tiles` together, because a
joined group and a one-launch group can launch equally often:
    one launch over the batches as they lie (`group_fold` = 1, joined span <= 24 x rows): launches and tiles equal those of the
        same group without its string column -- the same group table, the strings fold into the same launch (+ 0)
    joined on the device, then filtered as ONE batch (`group_fold` = 0, or span > 24 x rows): tiles equal those of
        filter_record on one batch of all the rows, launches exceed it by the filter_record difference above (+ 0 folded short
        strings, + 1 long ones); its tile count differs from the group table's, which has at least one tile per batch or packs waves
"""
import functools

import numpy as np
import pyarrow as pa
import pytest

import chapterhouseqe_amd as chq
from chapterhouseqe_amd import sqlast as A
from chapterhouseqe_amd.sqlparse import parse_expr

from . import utf8_reference as R

pytestmark = pytest.mark.gpu

N = R.N_GPU
PRED = parse_expr("sel = 1")
MAX_FOLD_UTF8 = 2   # device_program.h


# ---- inputs and their expected results, built once and shared (read-only) ----------------------------------------------------
def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _keep(selection, n):
    return _frozen(R.SELECTIONS[selection](n))[0]


@functools.lru_cache(maxsize=8)
def _column(profile, n=N, nulls=None, lead=0, first=None):
    """`nulls`: None, "bytes" (20 % nulls, their bytes kept) or "empty" (20 % nulls of length 0); `first`: the length of one
    extra row in front (the parent of a slice that starts at an odd byte)"""
    lengths = R.LENGTH_PROFILES[profile].lengths(n)
    valid = None
    if nulls:
        valid = np.random.default_rng(n + len(profile)).random(n) >= 0.2
        if nulls == "empty":
            lengths = np.where(valid, lengths, 0)
    if first is not None:
        lengths = np.concatenate([[first], lengths])
        valid = None if valid is None else np.concatenate([[True], valid])
    return R.make_utf8(lengths, valid=valid, lead=lead)


@functools.lru_cache(maxsize=80)
def _expected(selection, profile, n=N, nulls=None, lead=0):
    return _frozen(*R.expected_filter(_column(profile, n, nulls, lead), _keep(selection, n)))


def _side(arr):
    offsets, _, _ = R.utf8_parts(arr)
    return "short" if int(offsets[-1]) - int(offsets[0]) <= 24 * len(arr) else "long"


def _route_delta(options, arrays):
    """launches the string columns `arrays` add to a filter_record call under `options` (the table in the module docstring)"""
    folds = options.get("fold_utf8", 1) == 1 and options.get("tile_kind", -1) != 2
    delta = 0
    for k, arr in enumerate(arrays):
        short = _side(arr) == "short"
        delta += ((0 if short else 1) if folds and k < MAX_FOLD_UTF8 else (1 if short else 2)) + (1 if arr.null_count else 0)
    return delta


# ---- the device side -----------------------------------------------------------------------------------------------------------
def _context(options):
    ctx = chq.Context(0)
    for key, value in options.items():
        ctx.set_option(key, value)
    return ctx


class Staged:
    """The string columns and `id` staged once; `batch(keep)` puts a fresh `sel` column in front of them (the same buffers)."""

    def __init__(self, ctx, arrays, on_device=True):
        self.ctx, self.n, self.on_device = ctx, len(arrays[0]), on_device
        self.names = [f"s{k}" if k else "s" for k in range(len(arrays))] + ["id"]
        self.host = pa.RecordBatch.from_arrays(list(arrays) + [pa.array(np.arange(self.n, dtype=np.int32))], names=self.names)
        self.live = []
        if on_device:
            self.dev = chq.DeviceRecordBatch.from_host(self.host, ctx)
            self.cols = self.dev.describe_columns()

    def batch(self, keep, strings=True):
        sel = pa.array(np.asarray(keep).astype(np.int32))
        if not self.on_device:
            cols = list(self.host.columns) if strings else [self.host.column(self.host.num_columns - 1)]
            return pa.RecordBatch.from_arrays([sel] + cols, names=["sel"] + (self.names if strings else ["id"]))
        dsel = chq.DeviceRecordBatch.from_host(pa.RecordBatch.from_arrays([sel], names=["sel"]), self.ctx)
        cols = dsel.describe_columns() + (self.cols if strings else self.cols[-1:])
        out = chq.DeviceRecordBatch.from_device_buffers(cols, self.n, ctx=self.ctx, keepalive=[dsel, self.dev])
        self.live += [out, dsel]
        return out

    def release(self):
        for b in self.live:
            b.release()
        self.live = []
        if self.on_device:
            self.dev.release()


def _filter(ctx, batch, pred=PRED):
    """(the result on the host, the launches of the call)"""
    al = [[] for _ in range(batch.num_columns)]
    out = chq.filter_record(batch, al, pred, ctx=ctx)
    launches = ctx.last_stats()["launches"]
    if isinstance(out, pa.RecordBatch):
        return out, launches
    host = out.to_host()
    out.release()
    return host, launches


def _filter_group(ctx, batches):
    """(every batch's result on the host, (launches, tiles) of the call)"""
    outs = chq.filter_records(batches, [[] for _ in range(batches[0].num_columns)], PRED, ctx=ctx)
    stats = ctx.last_stats()
    hosts = [o.to_host() for o in outs]
    for o in outs:
        o.release()
    return hosts, (stats["launches"], stats["tiles"])


# ---- the comparison ------------------------------------------------------------------------------------------------------------
def check_utf8(col, want, what, joined=False):
    """offsets (all kept + 1 of them, the first 0), the bytes up to the last offset, validity and null count of a result column
    against (offsets, bytes, validity).  `joined`: the column is one batch's share of filter_records' joined result -- its
    offsets go on where the batch before it ended (compared relative to the first) and its bytes begin there."""
    w_off, w_data, w_valid = want
    assert pa.types.is_string(col.type) and len(col) == len(w_valid), f"{what}: {len(col)} rows, expected {len(w_valid)}"
    assert col.null_count == int((~w_valid).sum()), f"{what}: null count {col.null_count}, expected {int((~w_valid).sum())}"
    offsets, data, valid = R.utf8_parts(col)   # (asserts that the offsets buffer holds all len + 1 of them)
    assert joined or offsets[0] == 0, f"{what}: first offset {offsets[0]}"
    if len(col) == 0:
        return
    data, offsets = data[int(offsets[0]):], offsets - offsets[0]
    if not np.array_equal(offsets, w_off):
        k = int(np.flatnonzero(offsets != w_off)[0])
        raise AssertionError(f"{what}: offset {k} is {offsets[k]}, expected {w_off[k]} (output rows {len(col)})")
    got = data[:int(offsets[-1])]
    if not np.array_equal(got, w_data):
        b = int(np.flatnonzero(got != w_data)[0])
        row = int(np.searchsorted(offsets, b, side="right")) - 1
        lo = int(offsets[row])
        raise AssertionError(f"{what}: byte {b - lo} of output row {row} (length {int(offsets[row + 1]) - lo}) is "
                             f"{bytes(got[b:b + 8])!r}..., expected {bytes(w_data[b:b + 8])!r}...; {int((got != w_data).sum())} bytes differ")
    assert np.array_equal(valid, w_valid), f"{what}: validity differs at output row {int(np.flatnonzero(valid != w_valid)[0])}"


def check_result(got, keep, wants, what, first_id=0, joined=False):
    ids = first_id + np.flatnonzero(keep).astype(np.int32)
    assert got.num_rows == len(ids) and got.num_columns == len(wants) + 2, f"{what}: {got.num_rows} rows, expected {len(ids)}"
    assert got.column(got.num_columns - 1).null_count == 0 and np.array_equal(got.column(got.num_columns - 1).to_numpy(), ids), f"{what}: id"
    assert np.array_equal(got.column(0).to_numpy(), np.ones(len(ids), dtype=np.int32)), f"{what}: sel"
    for k, want in enumerate(wants):
        check_utf8(got.column(1 + k), want, f"{what}, column {k}", joined)


def run_selections(ctx, staged, options, arrays, wants_of, what, view=None, first_id=0, delta=None, selections=None):
    """every selection through one staged batch: result and launch difference.  `view`: (offset, length) of a device slice"""
    delta = _route_delta(options, arrays) if delta is None else delta
    cells = 0
    for name in selections or R.SELECTIONS:
        keep = _keep(name, staged.n)
        full, bare = staged.batch(keep), staged.batch(keep, strings=False)
        if view:
            full, bare = full.slice(*view), bare.slice(*view)
            keep = keep[view[0]:view[0] + view[1]]
        got, launches = _filter(ctx, full)
        _, base = _filter(ctx, bare)
        if view:
            full.release()
            bare.release()
        check_result(got, keep, wants_of(name), f"{what}, {name}", first_id)
        assert launches - base == delta, f"{what}, {name}: {launches} launches, {base} without the string columns, expected + {delta}"
        cells += 1
    return cells


# ---- the matrix: every profile x every selection through the routes of its kind ------------------------------------------------
ROUTES = {
    "fold-k0": {"fold_utf8": 1, "tile_kind": 0},
    "fold-k1": {"fold_utf8": 1, "tile_kind": 1},
    "followup-k0": {"fold_utf8": 0, "tile_kind": 0},
    "followup-k1": {"fold_utf8": 0, "tile_kind": 1},
    "followup-k2": {"fold_utf8": 0, "tile_kind": 2},
    "fold-k0-split": {"fold_utf8": 1, "tile_kind": 0, "split_rows": 1},        # FULL launch + tail launch
    "followup-k1-split": {"fold_utf8": 0, "tile_kind": 1, "split_rows": 1},
}


@pytest.mark.parametrize("profile,route", [(p, r) for p in R.LENGTH_PROFILES for r in ROUTES])
def test_profile_by_selection(profile, route):
    options = ROUTES[route]
    arr = _column(profile)
    assert _side(arr) == R.LENGTH_PROFILES[profile].side
    ctx = _context(options)
    try:
        staged = Staged(ctx, [arr])
        run_selections(ctx, staged, options, [arr], lambda sel: [_expected(sel, profile)], f"{profile} / {route}")
        staged.release()
    finally:
        ctx.close()


@pytest.mark.parametrize("tile_kind", [0, 1])
@pytest.mark.parametrize("profiles", [("cycle41", "const129", "const17"), ("const143", "mixed", "const257"), ("spike4", "group24_long", "group24_short")])
def test_third_utf8_column_takes_the_follow_up(profiles, tile_kind):
    """two columns ride in the main kernel (with their bytes, or offsets only + utf8_copy_kernel), the third takes
    utf8_filter_kernel or utf8_offsets_kernel + utf8_copy_kernel -- in one call"""
    options = {"fold_utf8": 1, "tile_kind": tile_kind}
    arrays = [_column(p) for p in profiles]
    ctx = _context(options)
    try:
        staged = Staged(ctx, arrays)
        run_selections(ctx, staged, options, arrays, lambda sel: [_expected(sel, p) for p in profiles], f"{profiles} / k{tile_kind}")
        staged.release()
    finally:
        ctx.close()


@pytest.mark.parametrize("route", ["fold-k0", "fold-k1", "followup-k0", "followup-k1", "followup-k2", "fold-k0-split"])
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_row_counts_around_one_group(n, route):
    options = ROUTES[route]
    ctx = _context(options)
    try:
        for profile in ("cycle41", "const129", "const16"):
            arr = _column(profile, n)
            staged = Staged(ctx, [arr])
            run_selections(ctx, staged, options, [arr], lambda sel: [_expected(sel, profile, n)], f"{profile} / {route} / {n} rows")
            staged.release()
    finally:
        ctx.close()


# ---- the uniform-length rewrite ---------------------------------------------------------------------------------------------------
def _uniform_case(ctx, arr, keep_rows, view, pred=PRED):
    """the results and launch counts of one batch with the rewrite on and off, and of the batch without its string column"""
    staged = Staged(ctx, [arr])
    keep = np.concatenate([np.zeros(view[0], dtype=bool), keep_rows])
    full, bare = staged.batch(keep).slice(*view), staged.batch(keep, strings=False).slice(*view)
    ctx.set_option("uniform_utf8_rows", 1)
    on = _filter(ctx, full, pred)
    base = _filter(ctx, bare)[1]
    ctx.set_option("uniform_utf8_rows", 0)
    off = _filter(ctx, full, pred)
    full.release()
    bare.release()
    staged.release()
    return on, off, base


@pytest.mark.parametrize("odd_start", [False, True])
@pytest.mark.parametrize("L", [1, 2, 4, 8, 16])
def test_uniform_rewrite(L, odd_start):
    """device input whose values all have one length: utf8_uniform_kernel proves it, the bytes go through the fixed-width copy,
    iota_offsets_kernel writes the offsets.  `odd_start`: a slice behind one 3-byte row of a parent whose offsets begin at 2 --
    the first value lies at byte 5."""
    profile = f"const{L}"
    arr = _column(profile, N, None, 2, 3) if odd_start else _column(profile)
    view = (1, N) if odd_start else (0, N)
    want_arr = arr.slice(*view)
    ctx = _context({})
    try:
        for name in R.SELECTIONS:
            keep = _keep(name, N)
            (got, launches), (ref, _), base = _uniform_case(ctx, arr, keep, view)
            want = R.expected_filter(want_arr, keep)
            check_result(got, keep, [want], f"uniform {L} / {name}", view[0])
            check_result(ref, keep, [want], f"uniform {L} off / {name}", view[0])
            assert launches - base == 2, f"uniform {L} / {name}: {launches} launches, {base} without the string column"
    finally:
        ctx.close()


def _refused_cases():
    n = N
    valid = np.ones(n, dtype=bool); valid[n - 70] = False
    ragged = np.full(n, 8); ragged[n - 7] = 5
    return {
        "length3": (R.make_utf8(np.full(n, 3)), PRED),
        "length24": (R.make_utf8(np.full(n, 24)), PRED),
        "one-other-length": (R.make_utf8(ragged), PRED),
        "one-null": (R.make_utf8(np.full(n, 8), valid=valid), PRED),
        "predicate-reads-it": (R.make_utf8(np.full(n, 8)), parse_expr("sel = 1 and s >= ''")),
    }


@pytest.mark.parametrize("case", ["length3", "length24", "one-other-length", "one-null", "predicate-reads-it"])
def test_uniform_rewrite_refused(case):
    """what the rewrite must leave alone: same result, and no launch more than with the rewrite switched off"""
    arr, pred = _refused_cases()[case]
    ctx = _context({})
    try:
        for name in R.SELECTIONS:
            keep = _keep(name, N)
            (got, launches), (ref, ref_launches), _ = _uniform_case(ctx, arr, keep, (0, N), pred)
            want = R.expected_filter(arr, keep)
            check_result(got, keep, [want], f"{case} / {name}")
            check_result(ref, keep, [want], f"{case} off / {name}")
            assert launches == ref_launches, f"{case} / {name}: {launches} launches, {ref_launches} with uniform_utf8_rows = 0"
    finally:
        ctx.close()


# ---- slices, host input, nulls ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["fold-k0", "fold-k1", "followup-k1", "followup-k2"])
@pytest.mark.parametrize("offset", [1, 63, 64, 4097])
@pytest.mark.parametrize("profile", ["cycle41", "const129"])
def test_sliced_device_view(profile, offset, route):
    """DeviceRecordBatch.slice of a parent whose offsets begin at byte 5: the view's rows start in mid-group, at any byte"""
    options = ROUTES[route]
    arr = _column(profile, N, None, 5)
    view = (offset, N - offset - 9)
    want_arr = arr.slice(*view)
    ctx = _context(options)
    try:
        staged = Staged(ctx, [arr])
        wants = lambda sel: [R.expected_filter(want_arr, _keep(sel, N)[view[0]:view[0] + view[1]])]
        run_selections(ctx, staged, options, [want_arr], wants, f"{profile} / slice {view} / {route}", view=view, first_id=offset)
        staged.release()
    finally:
        ctx.close()


@pytest.mark.parametrize("profile", ["cycle41", "const129"])
def test_host_input(profile):
    """a host pa.RecordBatch in, a host batch out: staged by the library, which then knows the byte span without a read-back.
    The one-block small-host path takes no Utf8 column (filter.cpp: plain_host_columns), so it is switched off: the call
    without the string column then goes the same way, staging + filter_record, and the launch difference compares like with like."""
    options = {"small_host": 0}
    arr = _column(profile, N, None, 3)
    ctx = _context(options)
    try:
        staged = Staged(ctx, [arr], on_device=False)
        run_selections(ctx, staged, options, [arr], lambda sel: [_expected(sel, profile, N, None, 3)], f"{profile} / host")
    finally:
        ctx.close()


@pytest.mark.parametrize("route", ["fold-k0", "fold-k1", "followup-k0", "followup-k2"])
@pytest.mark.parametrize("nulls", ["bytes", "empty"])
@pytest.mark.parametrize("profile", ["cycle41", "const129"])
def test_nulls(profile, nulls, route):
    """20 % nulls; a null slot keeps its bytes (they are copied like any row's) or is empty"""
    options = ROUTES[route]
    arr = _column(profile, N, nulls)
    assert arr.null_count > N // 10
    ctx = _context(options)
    try:
        staged = Staged(ctx, [arr])
        run_selections(ctx, staged, options, [arr], lambda sel: [_expected(sel, profile, N, nulls)], f"{profile} / nulls {nulls} / {route}")
        staged.release()
    finally:
        ctx.close()


# ---- batch groups ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group_mode", [0, 1, 2])
@pytest.mark.parametrize("group_fold", [1, 0])
@pytest.mark.parametrize("profile", ["cycle41", "const16", "const33"])
def test_batch_group(profile, group_fold, group_mode):
    """filter_records over 40 device batches of 1 000 .. 1 300 rows: the one-launch path (`group_fold`) reuses the fold, the
    other settings join on the device and filter one batch; every batch's result against the reference.  (The results are cut
    from one joined batch: only the first one's offsets begin at 0.)  Which of the two ran: the module docstring."""
    rows = [1000 + (37 * b) % 301 for b in range(40)]
    ctx = _context({"group_fold": group_fold, "group_mode": group_mode})
    try:
        parts = [Staged(ctx, [_column(profile, n, None, b % 4)]) for b, n in enumerate(rows)]
        joined = pa.concat_arrays([p.host.column(0) for p in parts])
        one_launch = group_fold == 1 and _side(joined) == "short"
        assert (_side(joined) == "short") == (profile != "const33")
        for name in R.SELECTIONS:
            keeps = [_keep(name, n) for n in rows]
            outs, (launches, tiles) = _filter_group(ctx, [p.batch(k) for p, k in zip(parts, keeps)])
            assert len(outs) == len(parts)
            for b, (p, k, got) in enumerate(zip(parts, keeps, outs)):
                check_result(got, k, [R.expected_filter(p.host.column(0), k)], f"{profile} / group / {name} / batch {b}", joined=True)
            # the same group without its string column, and one batch of all the rows through filter_record
            _, (bare_launches, bare_tiles) = _filter_group(ctx, [p.batch(k, strings=False) for p, k in zip(parts, keeps)])
            whole = pa.RecordBatch.from_arrays([pa.array(np.concatenate(keeps).astype(np.int32)), pa.array(np.arange(sum(rows), dtype=np.int32))],
                                               names=["sel", "id"])
            single = chq.DeviceRecordBatch.from_host(whole, ctx)
            chq.filter_record(single, [[], []], PRED, ctx=ctx).release()
            single_launches, single_tiles = ctx.last_stats()["launches"], ctx.last_stats()["tiles"]
            single.release()
            what = (f"{profile} / group / {name}: {launches} launches, {tiles} tiles; without the strings {bare_launches}, {bare_tiles}; "
                    f"one batch of {sum(rows)} rows {single_launches}, {single_tiles}")
            assert bare_tiles != single_tiles, what   # (else the two routes could not be told apart)
            if one_launch:
                assert (launches, tiles) == (bare_launches, bare_tiles), what
            else:
                assert (launches - single_launches, tiles) == (_route_delta({}, [joined]), single_tiles), what
        for p in parts:
            p.release()
    finally:
        ctx.close()


# ---- comparisons ---------------------------------------------------------------------------------------------------------------------
CMP_ROWS = 2 * 2048 + 37
CMP_LITERALS = [v for v in R.COMPARE_TABLE if R.is_utf8(v)]


def _cmp(op, left, right):
    return A.BinaryOp(left, A.BinaryOperator[op], right)


def _truth(op, left, right):
    """compare_bytes row by row as int8: 1 true, 0 false, -1 null"""
    return np.array([{True: 1, False: 0, None: -1}[R.compare_bytes(op, x, y)] for x, y in zip(left, right)], dtype=np.int8)


@pytest.mark.parametrize("variant", ["plain", "nulls-a", "nulls-b", "nulls-both", "sliced"])
@pytest.mark.parametrize("tile_kind", [1, 2])
def test_comparisons(tile_kind, variant):
    """all six operators: column against column, column against every UTF-8 literal of the table on either side (`'x' < a`:
    the reversed operand), with nulls in `a`, in `b` and in both, and on a slice that starts in mid-group.  What filter_record
    keeps are the rows where the comparison is true; compute_value shows false and null apart."""
    t = len(R.COMPARE_TABLE)
    first = 70 if variant == "sliced" else 0
    total = CMP_ROWS + first
    av, bv = R.compare_pairs(total)
    if variant in ("nulls-a", "nulls-both", "sliced"):
        av = [None if i % 7 == 3 else v for i, v in enumerate(av)]
    if variant in ("nulls-b", "nulls-both"):
        bv = [None if i % 5 == 1 else v for i, v in enumerate(bv)]
    rec = pa.RecordBatch.from_arrays([R.binary_column(av, lead=1), R.binary_column(bv), pa.array(np.arange(total, dtype=np.int32))],
                                     names=["a", "b", "id"])
    av, bv = av[first:], bv[first:]
    pair = (np.arange(first, total) % (t * t))          # row -> index into the crossed table: truth tables are built on 324 rows
    a_null = np.array([v is None for v in av])
    b_null = np.array([v is None for v in bv])
    ta, tb = R.compare_pairs(t * t)
    al = [[], [], []]
    ctx = _context({"tile_kind": tile_kind})
    try:
        parent = chq.DeviceRecordBatch.from_host(rec, ctx)
        dev = parent.slice(first, CMP_ROWS) if first else parent

        def kept(expr):
            out = chq.filter_record(dev, al, expr, ctx=ctx)
            host = out.to_host()
            out.release()
            return host.column(2).to_numpy()

        def rows_where_true(truth324, nulls):
            truth = truth324[pair].copy()
            truth[nulls] = -1
            return truth, first + np.flatnonzero(truth == 1).astype(np.int32)

        forms = 0
        for op in R.COMPARE_OPS:
            truth, want = rows_where_true(_truth(op, ta, tb), a_null | b_null)
            expr = _cmp(op, A.ident("a"), A.ident("b"))
            assert np.array_equal(kept(expr), want), f"a {op} b"
            value, scalar = chq.compute_value(dev, al, expr, ctx=ctx)
            got = np.array([{True: 1, False: 0, None: -1}[v] for v in value.to_pylist()], dtype=np.int8)
            assert not scalar and np.array_equal(got, truth), f"a {op} b (compute_value): rows {np.flatnonzero(got != truth)[:5]}"
            forms += 1
            for lit in CMP_LITERALS:
                node = A.string(lit.decode())
                _, want = rows_where_true(_truth(op, ta, [lit] * len(ta)), a_null)
                assert np.array_equal(kept(_cmp(op, A.ident("a"), node)), want), f"a {op} {lit!r}"
                _, want = rows_where_true(_truth(op, [lit] * len(ta), ta), a_null)
                assert np.array_equal(kept(_cmp(op, node, A.ident("a"))), want), f"{lit!r} {op} a"
                forms += 2
        assert forms == 6 * (1 + 2 * len(CMP_LITERALS)) and len(CMP_LITERALS) == t - 2

        # five literals: more than one program holds (MAX_CONST_STR = 4)
        five = [b"", b"a\x00", b"ab", "é".encode(), R.COMPARE_TABLE[13]]
        expr = None
        for lit in five:
            eq = _cmp("Eq", A.ident("a"), A.string(lit.decode()))
            expr = eq if expr is None else A.BinaryOp(expr, A.BinaryOperator.Or, eq)
        want = first + np.flatnonzero(np.array([v in five for v in av])).astype(np.int32)
        assert np.array_equal(kept(expr), want), "a = l1 or .. or a = l5"

        # a literal comparison and a column comparison in one predicate
        expr = A.BinaryOp(_cmp("GtEq", A.ident("a"), A.string("ab")), A.BinaryOperator.And, _cmp("Lt", A.ident("b"), A.ident("a")))
        want = first + np.flatnonzero(np.array([x is not None and y is not None and x >= b"ab" and y < x for x, y in zip(av, bv)])).astype(np.int32)
        assert np.array_equal(kept(expr), want), "a >= 'ab' and b < a"
        if first:
            dev.release()
        parent.release()
    finally:
        ctx.close()
