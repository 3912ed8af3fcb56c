"""An independent model of the batch-group filter's host plans (csrc/group_plan.cpp), written from DESIGN.md (the batch-group
launch) and the comments of device_program.h (FilterParams::group, BitCompactGroupParams), not from the C++.  The CPU tier
(tests/test_group_plan_host.py) compares every plan of tests/group_plan_main.cpp with it; the GPU tier
(tests/test_gpu_group.py) compares `tiles` and `launches` of a real call with `predict_launch`.

A schema is a string with one letter per column: `f` fixed-width, `u` Utf8, `b` Boolean."""
from fractions import Fraction
from functools import lru_cache

MAX_REFS, MAX_OUT, MAX_FOLD_UTF8 = 12, 40, 2
ROWS_PER_LANE = (16, 8, 8)          # R of the three tile kinds
WAVES_PER_TILE = (16, 4, 4)         # workgroups of 1024 / 256 / 256 lanes
WAVE_ROWS = tuple(64 * r for r in ROWS_PER_LANE)
TILE_ROWS = tuple(w * n for w, n in zip(WAVE_ROWS, WAVES_PER_TILE))
BIT_COUNTERS = 16                   # null counters a launch has for its bit columns
ROW_LIMIT = 2**31 - 64              # rows (waves) one launch addresses
CHUNK_ROWS = 2**30


def ceil_div(a, b):
    return -(-a // b)


def eligibility(schema, short, differs, on_host, on_device, nulls, no_data, opts):
    """the verdict over a group: `short`, `differs`, `nulls`, `no_data` say whether ANY batch has the property, `on_host` /
    `on_device` whether ALL batches lie there; `opts` has group_bits, fold_utf8, group_fold; host_in = batch 0 in host memory"""
    if short or differs:
        return {"per_batch": True}
    fits = len(schema) <= MAX_OUT
    need_bits = "b" in schema or nulls
    bits_allowed = not need_bits or bool(opts["group_bits"])
    plain = fits and "u" not in schema and (not need_bits or (on_device and bits_allowed))
    n_utf8 = schema.count("u")
    fold = (not plain and fits and bool(opts["fold_utf8"]) and bool(opts["group_fold"]) and on_device and not no_data and bits_allowed
            and 1 <= n_utf8 <= MAX_FOLD_UTF8 and opts["total_rows"] < ROW_LIMIT)
    return {"per_batch": False, "plain": plain, "fold": fold, "need_bits": need_bits, "resident": on_host if opts["host_in"] else on_device,
            "n_fold": n_utf8 if fold else 0}


@lru_cache(maxsize=None)
def tiling(rows, wide, tile_kind, mode):
    """(tile kind, waves per batch or 0 for the per-tile table, tiles) of a group with these rows per batch (a tuple)"""
    nb, total, longest = len(rows), sum(rows), max(rows)
    kind = 2 if wide else tile_kind          # wide value classes / temporaries have one instantiation only
    k = max(kind, 0)
    wpb = ceil_div(longest, WAVE_ROWS[k])     # every batch gets the wave count of the longest one
    # near-uniform: at most a fifth of the lanes of the packed launch idle, i.e. the padded rows are within 5/4 of the real ones
    packed = Fraction(wpb * nb * WAVE_ROWS[k], total) <= Fraction(5, 4) and wpb * nb < ROW_LIMIT
    if mode == 2 or (mode == 0 and packed):
        return k, wpb, ceil_div(wpb * nb, WAVES_PER_TILE[k])
    if kind < 0:   # the large tile unless whole large tiles per batch idle more than a quarter
        kind = 0 if Fraction(sum(ceil_div(r, TILE_ROWS[0]) * TILE_ROWS[0] for r in rows), total) <= Fraction(5, 4) else 1
    return kind, 0, sum(ceil_div(r, TILE_ROWS[kind]) for r in rows)


def table_layout(kind, wpb, ntiles, nb, n_refs, n_out, n_fold, need_bits, n_bit_cols):
    """None (declined) or (stride, bits_at, table rows, bytes of table, index, end offsets)"""
    if need_bits and (wpb == 0 or n_bit_cols > BIT_COUNTERS):
        return None
    if n_fold and kind == 2:
        return None
    # {rows} or {first row, rows}; value pointers of the refs; input pointers of the outputs; offsets and bytes per folded column
    stride = (1 if wpb else 2) + n_refs + n_out + 2 * n_fold
    bits_at = 0
    if need_bits:   # bitmap and bit position per ref, then a pair per bit column
        bits_at = stride
        stride += 2 * n_refs + 2 * n_bit_cols
    table_rows = nb if wpb else ntiles
    return stride, bits_at, table_rows, 8 * stride * table_rows, 0 if wpb else 8 * nb, 8 * nb


def fold_verdict(caps, total_rows, chunk_bytes):
    """(fits one output column, short strings)"""
    short = all(cap <= 24 * total_rows for cap in caps)
    return short and all(cap < 2 * chunk_bytes - 64 for cap in caps), short


@lru_cache(maxsize=None)
def cuts(rows, bytes_per_column, limit):
    """greedy chunks: a new chunk starts at the batch that would take the rows past 2^30 or any column's bytes past `limit`"""
    out, at = [0], 0
    sums = [0] * len(bytes_per_column)
    for b, r in enumerate(rows):
        over = at + r > CHUNK_ROWS or any(s + col[b] > limit for s, col in zip(sums, bytes_per_column))
        if over and b > out[-1]:
            out.append(b)
            at, sums = 0, [0] * len(bytes_per_column)
        at += r
        sums = [s + col[b] for s, col in zip(sums, bytes_per_column)]
    return tuple(out + [len(rows)])


def sub_groups(c):
    return len(c) > 2 and all(b - a >= 2 for a, b in zip(c, c[1:]))


def concat_words(schema, nb, null_cols):
    """words of the concat kernels' tables: row starts, then per column its sources, for Utf8 the byte buffers and running byte
    positions, for Boolean the bit offsets, for a column with nulls the bitmaps and their bit offsets"""
    words = nb + 1
    for i, kind in enumerate(schema):
        words += nb + {"u": nb + nb + 1, "b": nb, "f": 0}[kind] + (2 * nb if i in null_cols else 0)
    return words


def predict_launch(rows, schema, null_cols=(), tile_kind=-1, mode=0, n_refs=1):
    """{"tiles", "launches"} of one filter_records call over a device-resident group whose predicate reads fixed-width columns
    and whose strings are short -- or None where the one-launch path declines"""
    rows = tuple(rows)
    e = eligibility(schema, min(rows) < 2, False, False, True, bool(null_cols), False,
                    {"group_bits": 1, "fold_utf8": 1, "group_fold": 1, "host_in": False, "total_rows": sum(rows)})
    if e["per_batch"] or not (e["plain"] or e["fold"]):
        return None
    kind, wpb, ntiles = tiling(rows, False, tile_kind, mode)
    n_bit_cols = (schema.count("b") + len(null_cols)) if e["need_bits"] else 0
    if table_layout(kind, wpb, ntiles, len(rows), n_refs, schema.count("f"), e["n_fold"], e["need_bits"], n_bit_cols) is None:
        return None
    # the main kernel; the per-tile table needs the end offsets gathered from the status words; one compaction per bit column
    return {"tiles": ntiles, "launches": 1 + (0 if wpb else 1) + n_bit_cols}
