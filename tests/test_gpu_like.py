"""GPU: LIKE / NOT LIKE / IS [NOT] NULL on the device (like.hip, typed_ops.hip: is_null_kernel) -- every row of every case
against tests/like_reference.py, which the CPU tier pins to sqlite3 and pyarrow.compute.match_like.  Inside predicates the
new nodes are checked through the existing yardstick: the predicate is projected into a Boolean column `m` (the path the
first half of this file checks), `m` is appended to the batch, and the CPU oracle filters with `m and ...` / `m or ...`."""
import os
import re

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest

import chapterhouseqe_amd as chq
from chapterhouseqe_amd import sqlast as A
from chapterhouseqe_amd.sqlparse import parse_expr, parse_select
from oracle import oracle as O

from . import like_reference as R
from .cases import empty_aliases
from .helpers import batches_identical, explain_diff

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_HDR = open(os.path.join(ROOT, "chapterhouseqe_amd", "csrc", "like_device.h")).read()
# like.hip: a wave whose 64 rows hold MORE than this many string bytes walks them one at a time, 64 candidate positions per step
WAVE_MODE_BYTES = int(re.search(r"LIKE_WAVE_MODE_BYTES\s*=\s*(\d+)", _HDR).group(1))
STEP = 64
GRID_ROWS = 256 * 32 * 256   # rows one pass of the launch grid covers (typed_ops.hip, like.hip: the cap of rows_grid)

# (pattern, escape): the fixed table of the CPU tier, the escape forms, and forms with several pieces to search for
PATTERNS = [(p, None) for p in R.PATTERNS] + [("h_llo", None), ("%é_", None), ("_本%", None), ("%a_b%", None), ("%ab%b", None), ("a%\n%", None),
                                              ("%!%", "!"), ("a!_b", "!"), ("%!!%", "!"), ("_%%_", "%"), ("%a%b%a%", None), ("_%a_%_b", None)]
POOL = R.STRINGS + ["aXbXc", "abb", "abab", "aabab", "baab", "xab", "abx", "a%b", "a!b", "100%", "é_", "éé", "日本", "本語x", "a\nb\n", "ab" * 9,
                    "b" * 17 + "a", "a" + "b" * 17, "aab" * 5 + "a"]


@pytest.fixture(scope="module")
def ctx():
    c = chq.Context(0)
    yield c
    c.close()


def strings_batch(values, seed=0):
    """s Utf8 (as given, None = null), id Int32 0..n-1 with nulls, f Float32 with nulls"""
    n = len(values)
    rng = np.random.default_rng(seed)
    return pa.RecordBatch.from_arrays(
        [pa.array(values, pa.utf8()),
         pa.array(np.arange(n, dtype=np.int32), mask=(rng.random(n) < 0.2) if n else None),
         pa.array((rng.random(n) * 2).astype(np.float32), mask=(rng.random(n) < 0.2) if n else None)], names=["s", "id", "f"])


def pool_values(n, nulls, seed):
    rng = np.random.default_rng(seed)
    vals = [POOL[(i * 7 + seed) % len(POOL)] for i in range(n)]
    if nulls:
        vals = [None if rng.random() < 0.3 else v for v in vals]
        if n:
            vals[n // 2] = None
    return vals


def check_value(c, rec, host, sql, want, what):
    """compute_value of `sql` over `rec` (device or host record) against the list `want`, every row"""
    arr, is_scalar = chq.compute_value(rec, empty_aliases(host), parse_expr(sql), ctx=c)
    assert arr.type == pa.bool_() and not is_scalar, (what, sql)
    got = arr.to_pylist()
    if got != want:
        bad = [i for i in range(min(len(got), len(want))) if got[i] != want[i]][:8]
        raise AssertionError(f"{what}: {sql!r}: {len(got)} rows vs {len(want)}; first differences at {bad}: "
                             f"{[(host.column(0)[i].as_py(), got[i], want[i]) for i in bad]}")


def check_patterns(c, rec, host, patterns, what):
    """`s like P`, `s not like P`, `s is [not] null` for every pattern: compute_value one by one, then all four in ONE
    project_record (whose fields must come out nullable exactly when they hold a null, IS NULL never)"""
    s = host.column("s")
    strings = s.to_pylist()
    al = empty_aliases(host)
    nulls = s.null_count
    for p, esc in patterns:
        want = R.like_values(strings, p, esc)
        neg = R.like_values(strings, p, esc, negated=True)
        check_value(c, rec, host, R.like_sql("s", p, esc), want, what)
        check_value(c, rec, host, R.like_sql("s", p, esc, negated=True), neg, what)
        sel = parse_select(f"select {R.like_sql('s', p, esc)} as m, {R.like_sql('(s)', p, esc, negated=True)} as nm, s is null as z, "
                           "s is not null as nz, id is null as iz from t")
        out = chq.project_record(sel.projection, rec, al, ctx=c, device_result=False)
        assert out.schema.names == ["m", "nm", "z", "nz", "iz"] and all(f.type == pa.bool_() for f in out.schema), (what, p)
        assert out.column(0).to_pylist() == want and out.column(1).to_pylist() == neg, (what, p, esc)
        assert out.column(2).to_pylist() == [v is None for v in strings] and out.column(3).to_pylist() == [v is not None for v in strings], (what, p)
        assert out.column(4).to_pylist() == [v is None for v in host.column("id").to_pylist()], (what, p)
        assert [f.nullable for f in out.schema] == [nulls > 0, nulls > 0, False, False, False], (what, p, out.schema)
    check_value(c, rec, host, "s is null", [v is None for v in strings], what)
    check_value(c, rec, host, "s is not null", [v is not None for v in strings], what)
    # operands that are not bare columns: a computed one is materialised first, a LIKE is itself a temporary column
    ids = host.column("id").to_pylist()
    check_value(c, rec, host, "id + 1 is null", [v is None for v in ids], what)
    check_value(c, rec, host, "(id * 2 > 6) is not null", [v is not None for v in ids], what)
    check_value(c, rec, host, "s like '%a%' is null", [v is None for v in strings], what)
    check_value(c, rec, host, "(s not like 'a%') is not null and id is null", [v is not None and w is None for v, w in zip(strings, ids)], what)


# ---- the pattern table over the row counts of one wave, one block and more --------------------------------------------
@pytest.mark.parametrize("nulls", [False, True], ids=["dense", "nulls"])
@pytest.mark.parametrize("rows", [0, 1, 63, 64, 65, 257])
def test_pattern_table(ctx, rows, nulls):
    host = strings_batch(pool_values(rows, nulls, rows + 1), rows)
    dev = chq.DeviceRecordBatch.from_host(host, ctx)
    check_patterns(ctx, dev, host, PATTERNS, f"{rows} rows")
    check_patterns(ctx, host, host, PATTERNS[::5], f"{rows} rows, host record")


def raw_utf8(lengths, data, valid=None):
    offs = np.zeros(len(lengths) + 1, np.int32)
    np.cumsum(lengths, out=offs[1:])
    nulls = 0 if valid is None else int((~valid).sum())
    bitmap = pa.py_buffer(np.packbits(valid, bitorder="little").tobytes()) if nulls else None
    arr = pa.Array.from_buffers(pa.utf8(), len(lengths), [bitmap, pa.py_buffer(offs.tobytes()), pa.py_buffer(bytes(data))], null_count=nulls)
    arr.validate(full=True)
    return arr


@pytest.mark.parametrize("nulls", [False, True], ids=["dense", "nulls"])
def test_more_rows_than_one_grid_pass(ctx, nulls):
    """2^21 + 65 rows of 0..3 bytes: the grid-stride loop's second pass, and its last partial wave.  (Expected values from
    match_like, which the CPU tier pins to the reference on these patterns.)"""
    n = GRID_ROWS + 65
    rng = np.random.default_rng(5)
    lengths = rng.integers(0, 4, n)
    data = rng.choice(np.frombuffer(b"abc", np.uint8), int(lengths.sum())).tobytes()
    valid = rng.random(n) < 0.9 if nulls else None
    s = raw_utf8(lengths, data, valid)
    host = pa.RecordBatch.from_arrays([s], names=["s"])
    dev = chq.DeviceRecordBatch.from_host(host, ctx)
    for p in ["a%", "%a", "%a%", "_%_", "a%b", "%b_", "ab", ""]:
        for negated in (False, True):
            want = pc.match_like(s, p)
            want = pc.invert(want) if negated else want
            got, _ = chq.compute_value(dev, [[]], parse_expr(R.like_sql("s", p, None, negated)), ctx=ctx)
            assert got.null_count == want.null_count and got.equals(want), (p, negated, pc.sum(pc.xor(got.fill_null(False), want.fill_null(False))))
    got, _ = chq.compute_value(dev, [[]], parse_expr("s is null"), ctx=ctx)
    assert got.null_count == 0 and got.equals(pc.is_null(s))
    got, _ = chq.compute_value(dev, [[]], parse_expr("s is not null"), ctx=ctx)
    assert got.null_count == 0 and got.equals(pc.is_valid(s))


# ---- the string shapes ------------------------------------------------------------------------------------------------------
SHAPES = {
    "empty": ["", "", "", ""],
    "one byte": ["a", "b", "%", "_", "\n", "x"],
    "shorter than the pattern": ["a", "ab", "", "aa", "é", "b"],
    "only at the start": ["abxxxx", "aabxxx", "abbbbb", "ab", "xab", "abxab"],
    "only at the end": ["xxxxab", "xxxaab", "bbbbab", "ab", "abx", "abxab"],
    "overlapping partial matches": ["aaab", "aabaab", "ababab", "aaaaab", "abaabaaab", "aabab", "abab", "abaab", "aab", "aaaa"],
    "multibyte next to _": ["héllo", "hllo", "hééllo", "é", "éé", "aé", "éa", "日本語", "a日b", "日", "hé", "héllo"],
}
SHAPE_PATTERNS = [("ab%", None), ("%ab", None), ("%ab%", None), ("%aab%", None), ("%ab%ab%", None), ("abc%", None), ("%abc", None), ("a_c", None),
                  ("h_llo", None), ("_", None), ("__", None), ("%_", None), ("_%", None), ("a_", None), ("_a", None), ("%é%", None), ("_本_", None), ("a_b", None),
                  ("", None), ("%", None), ("%aa%ab%", None), ("aa%ab", None)]


@pytest.mark.parametrize("nulls", [False, True], ids=["dense", "nulls"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_string_shapes(ctx, shape, nulls):
    vals = list(SHAPES[shape]) * 12          # 48 .. 144 rows: within one wave and over several
    if nulls:
        vals = [None if i % 5 == 2 else v for i, v in enumerate(vals)]
    host = strings_batch(vals, 3)
    check_patterns(ctx, chq.DeviceRecordBatch.from_host(host, ctx), host, SHAPE_PATTERNS, shape)


def test_null_slots_enclosing_garbage(ctx):
    """null slots whose offsets enclose bytes: some that would match, some that would not, some of broken UTF-8"""
    cells = [b"ab", b"abab", b"xx", b"\xff\xfe", b"\x80\x80ab", b"a", b"", b"ab" * 40]
    n = 130
    rng = np.random.default_rng(9)
    pick = rng.integers(0, len(cells), n)
    valid = rng.random(n) < 0.5
    # broken bytes only in null slots (a valid slot is valid UTF-8)
    pick = np.where(valid & ((pick == 3) | (pick == 4)), 0, pick)
    valid[0], valid[1], valid[64], valid[65], valid[n - 1] = False, True, False, True, False
    pick[0], pick[64], pick[n - 1] = 1, 4, 7
    s = pa.Array.from_buffers(pa.utf8(), n, [pa.py_buffer(np.packbits(valid, bitorder="little").tobytes()),
                                            pa.py_buffer(np.concatenate([[0], np.cumsum([len(cells[k]) for k in pick])]).astype(np.int32).tobytes()),
                                            pa.py_buffer(b"".join(cells[k] for k in pick))], null_count=int((~valid).sum()))
    host = pa.RecordBatch.from_arrays([s, pa.array(np.arange(n, dtype=np.int32)), pa.array(np.zeros(n, np.float32))], names=["s", "id", "f"])
    assert host.column(0).to_pylist()[0] is None and host.column(0).to_pylist()[1] is not None
    check_patterns(ctx, chq.DeviceRecordBatch.from_host(host, ctx), host, [("ab%", None), ("%ab", None), ("%ab%", None), ("%ab%ab%", None), ("_%", None), ("%", None), ("", None)],
                   "null slots with bytes")


@pytest.mark.parametrize("nulls", [False, True], ids=["dense", "nulls"])
@pytest.mark.parametrize("rows", [1, 64, 100])
def test_all_empty_column_without_a_data_buffer(ctx, rows, nulls):
    """a caller-owned Utf8 column whose offsets are all equal and whose data pointer is null; its validity bitmap, when it has
    one, is a Boolean column's value bitmap uploaded beside it"""
    valid = np.arange(rows + 1) % 3 != 1
    ids = pa.RecordBatch.from_arrays([pa.array(np.zeros(rows + 1, np.int32)), pa.array(np.arange(rows + 1, dtype=np.int32)),
                                      pa.array(np.zeros(rows + 1, np.float32)), pa.array(valid)], names=["o", "id", "f", "v"])
    up = chq.DeviceRecordBatch.from_host(ids, ctx)
    s_desc = {"name": "s", "format": "u", "values": up.column_buffer_address(0)}
    if nulls:
        s_desc.update(validity=up.column_buffer_address(3), null_count=int((~valid[:rows]).sum()), nullable=True)
    dev = chq.DeviceRecordBatch.from_device_buffers([s_desc, {"name": "id", "format": "i", "values": up.column_buffer_address(1)},
                                                     {"name": "f", "format": "f", "values": up.column_buffer_address(2)}], rows, ctx, keepalive=[up])
    assert dev.column_buffer_address(0, 2) == 0
    strings = [("" if ok or not nulls else None) for ok in valid[:rows]]
    host = pa.RecordBatch.from_arrays([pa.array(strings, pa.utf8()), ids.column(1).slice(0, rows), ids.column(2).slice(0, rows)], names=["s", "id", "f"])
    pats = [("", None), ("%", None), ("%%", None), ("_", None), ("a%", None), ("%a%", None), ("%_%", None), ("%a%b%", None)]
    check_patterns(ctx, dev, host, pats, "no data buffer")


# ---- sliced device views ------------------------------------------------------------------------------------------------------
VIEW_WINDOWS = [(0, 300), (1, 299), (3, 100), (7, 64), (9, 65), (63, 2), (64, 64), (65, 130), (77, 0), (100, 1), (129, 171), (200, 63)]


def test_sliced_device_views(ctx):
    """row offsets that are no multiple of 8 or 64 (the validity bit offset), offsets[0] != 0, nulls inside and outside the
    window; and the same windows as host slices"""
    vals = pool_values(300, True, 11)
    for i in range(120, 160):          # a stretch without nulls: windows with a bitmap but no null inside
        vals[i] = POOL[i % len(POOL)]
    vals[0] = "ab"                       # offsets[0] of every later window is not 0
    host = strings_batch(vals, 4)
    dev = chq.DeviceRecordBatch.from_host(host, ctx)
    pats = [("a%", None), ("%a", None), ("%ab%", None), ("%ab%ab%", None), ("_%_", None), ("h_llo", None), ("%", None), ("", None), ("%!%", "!")]
    for off, ln in VIEW_WINDOWS:
        check_patterns(ctx, dev.slice(off, ln), host.slice(off, ln), pats, f"device view ({off}, {ln})")
    for off, ln in VIEW_WINDOWS[2::3]:
        check_patterns(ctx, host.slice(off, ln), host.slice(off, ln), pats[:4], f"host slice ({off}, {ln})")
    inner = dev.slice(120, 40)           # a bitmap rides along, no null inside
    out = chq.project_record(parse_select("select s like '%a%' as m, s is null as z from t").projection, inner, empty_aliases(host), ctx=ctx, device_result=False)
    assert [f.nullable for f in out.schema] == [False, False] and out.column(1).to_pylist() == [False] * 40


# ---- the wave-per-row mode ----------------------------------------------------------------------------------------------------
WAVE_PATTERNS = [("%ab%", None), ("%ab%b", None), ("%ab%ba%", None), ("%x_b%", None), ("%_b%", None), ("q%ab%", None), ("%aab%", None), ("%ab%ab%", None),
                 ("%a_b%é%", None), ("%é_é%", None), ("ab%", None), ("%ab", None), ("%", None), ("%zzzz%q%", None)]
FILLER = "z" * (WAVE_MODE_BYTES + 1)     # one such row puts its wave into the wave-per-row mode whatever the others hold


def wave_batch(rows64, nulls=False):
    """exactly 64 rows (one wave)"""
    assert len(rows64) == 64
    vals = list(rows64)
    if nulls:
        vals = [None if i % 7 == 3 else v for i, v in enumerate(vals)]
    return strings_batch(vals, 6)


@pytest.mark.parametrize("nulls", [False, True], ids=["dense", "nulls"])
def test_wave_mode_threshold(ctx, nulls):
    """64 rows holding exactly the threshold (lane per row), one byte more (wave per row), and much more"""
    rng = np.random.default_rng(21)
    per = WAVE_MODE_BYTES // 64
    rows = ["".join(rng.choice(list("ab"), per)) for _ in range(64)]
    rows[-1] += "a" * (WAVE_MODE_BYTES - 64 * per)
    for extra, what in ((0, "at the threshold"), (1, "one byte over"), (WAVE_MODE_BYTES, "far over")):
        vals = list(rows)
        vals[17] = vals[17] + "b" * extra
        host = wave_batch(vals, False)
        assert sum(len(v.encode()) for v in vals) == WAVE_MODE_BYTES + extra
        host = wave_batch(vals, nulls)
        check_patterns(ctx, chq.DeviceRecordBatch.from_host(host, ctx), host, WAVE_PATTERNS + [("%abab_b%aa%", None), ("%bbbbbbbbbbbb", None)], what)


@pytest.mark.parametrize("nulls", [False, True], ids=["dense", "nulls"])
def test_wave_mode_step_boundaries(ctx, nulls):
    """one long string among short ones; pieces that start at position 63 and 64 of a step, in the last partial step, two hits
    in one step of which only the leftmost may be taken, multibyte characters across a step boundary under `_`"""
    x = "x"
    rows = [FILLER,
            x * 63 + "ab",                             # the literal straddles the first step's end
            x * 64 + "ab",                             # ... starts the second step
            x * 62 + "ab",                             # ... ends the first step
            x * (STEP + 63) + "ab" + x * 70,           # the same one step later
            x * (STEP + 64) + "ab" + x * 70,
            x * (3 * STEP + 5) + "ab",                 # only in the last, partial step
            x * (3 * STEP + 5) + "a",                  # nowhere
            x * 10 + "ab" + x * 10 + "ab",             # %ab%b: no b behind the second hit
            x * 10 + "ab" + x * 10 + "abb",
            x * 10 + "ab" + x * 5 + "ba" + x * 5 + "ab",   # %ab%ba%: two hits of `ab` in one step, `ba` only behind the first
            x * 10 + "ab" + x * 5 + "ab" + x * 5 + "ba" + x * 200,
            x * 10 + "ba" + x * 5 + "ab",                  # `ba` only in front of `ab`
            "abab", "abb", "ab", "b", "",
            x * 62 + "xéb",                            # é = bytes 63 and 64: across the step boundary, under `_` of %x_b%
            x * 63 + "éb" + x * 80,                    # %_b%: a candidate on é's first byte (a hit) and on its second (never)
            x * 61 + "aébyé",                          # %a_b%é%
            x * 62 + "é" + "xé" + x * 3,               # %é_é%: the first é across the boundary
            x * 126 + "éaé",
            "q" + x * 62 + "ab", "q" + x * 63 + "ab", x + "q" + x * 62 + "ab",   # an anchored first piece moves the steps by one
            x * 200 + "aab" + x * 200, "a" * 63 + "ab", "a" * 64 + "b", "aab" * 40 + "ab",
            "zzzz" * 30 + "q", "zzz" * 50 + "q"]
    rows += [POOL[i % len(POOL)] for i in range(64 - len(rows))]
    assert len(rows) == 64
    host = wave_batch(rows, nulls)
    check_patterns(ctx, chq.DeviceRecordBatch.from_host(host, ctx), host, WAVE_PATTERNS, "step boundaries")
    # the same rows behind a wave of short strings (lane per row) and in front of a partial wave: the mode is per wave
    many = [POOL[i % len(POOL)] for i in range(64)] + rows + rows[1:40]
    host = strings_batch([None if nulls and i % 9 == 1 else v for i, v in enumerate(many)], 8)
    dev = chq.DeviceRecordBatch.from_host(host, ctx)
    check_patterns(ctx, dev, host, WAVE_PATTERNS[:8], "three waves")
    check_patterns(ctx, dev.slice(5, 150), host.slice(5, 150), WAVE_PATTERNS[:8], "three waves, view")


# ---- inside predicates: the existing yardstick -------------------------------------------------------------------------------------
PREDICATES = [("s like '%ab%'", "{m} and id > 5"), ("s like 'a%'", "{m} or f < 1.0"), ("s is null", "{m} or id = 3"),
              ("s not like '%a_b%'", "{m} and f < 1.5"), ("s is not null", "{m} and id > 5"), ("s like '%!%' escape '!'", "id > 5 or {m}")]


def with_mask(c, host, mask_sql):
    """`host` plus the Boolean column `m` = `mask_sql`, computed on the device"""
    out = chq.project_record(parse_select(f"select {mask_sql} as m from t").projection, chq.DeviceRecordBatch.from_host(host, c), empty_aliases(host),
                             ctx=c, device_result=False)
    m = out.column(0)
    return pa.RecordBatch.from_arrays(list(host.columns) + [m], schema=host.schema.append(pa.field("m", pa.bool_(), m.null_count > 0)))


def oracle_rows(c, host, mask_sql, shape):
    plus = with_mask(c, host, mask_sql)
    kept = O.filter_record(plus, empty_aliases(plus), parse_expr(shape.format(m="m")))
    return kept.drop_columns(["m"]) if hasattr(kept, "drop_columns") else pa.RecordBatch.from_arrays(kept.columns[:-1], schema=host.schema)


def predicate_batches():
    out = []
    for k, n in enumerate((257, 64, 1, 0, 130)):
        out.append(strings_batch(pool_values(n, True, 30 + k), 40 + k))
    return out


@pytest.mark.parametrize("mask_sql,shape", PREDICATES)
def test_filter_record_with_the_new_predicates(ctx, mask_sql, shape):
    sql = shape.format(m=mask_sql)
    for host in predicate_batches():
        want = oracle_rows(ctx, host, mask_sql, shape)
        al = empty_aliases(host)
        got = chq.filter_record(chq.DeviceRecordBatch.from_host(host, ctx), al, parse_expr(sql), ctx=ctx).to_host()
        assert batches_identical(got, want), f"{sql}, {host.num_rows} rows:\n{explain_diff(got, want)}"
        got = chq.filter_record(host, al, parse_expr(sql), ctx=ctx)
        assert batches_identical(got, want), f"{sql}, {host.num_rows} rows, host record:\n{explain_diff(got, want)}"


@pytest.mark.parametrize("mask_sql,shape", PREDICATES[:3])
def test_filter_records_with_the_new_predicates(ctx, mask_sql, shape):
    sql = shape.format(m=mask_sql)
    hosts = predicate_batches()
    want = [oracle_rows(ctx, h, mask_sql, shape) for h in hosts]
    al = empty_aliases(hosts[0])
    got = chq.filter_records([chq.DeviceRecordBatch.from_host(h, ctx) for h in hosts], al, parse_expr(sql), ctx=ctx)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert batches_identical(g.to_host(), w), f"{sql}, batch {i}:\n{explain_diff(g.to_host(), w)}"
    got = chq.filter_records(hosts, al, parse_expr(sql), ctx=ctx, device_result=False)
    for i, (g, w) in enumerate(zip(got, want)):
        assert batches_identical(g, w), f"{sql}, host batch {i}:\n{explain_diff(g, w)}"


@pytest.mark.parametrize("mask_sql,shape", PREDICATES[:3])
def test_filter_project_record_with_the_new_predicates(ctx, mask_sql, shape):
    sql = shape.format(m=mask_sql)
    fields = parse_select("select id, s, f + 1.0 as f1 from t").projection
    for host in predicate_batches():
        al = empty_aliases(host)
        want = O.project_record(fields, oracle_rows(ctx, host, mask_sql, shape), al)
        got = chq.filter_project_record(parse_expr(sql), fields, chq.DeviceRecordBatch.from_host(host, ctx), al, ctx=ctx).to_host()
        assert batches_identical(got, want), f"{sql}, {host.num_rows} rows:\n{explain_diff(got, want)}"


def test_is_null_after_a_left_join_is_the_anti_join(ctx):
    """a producer of nulls on the device: LEFT JOIN filtered by `rk is null` = the ANTI join of the same inputs"""
    rng = np.random.default_rng(77)
    nl, nr = 500, 200
    left = pa.RecordBatch.from_arrays([pa.array(rng.integers(0, 300, nl).astype(np.int32), mask=rng.random(nl) < 0.1),
                                       pa.array([POOL[i % len(POOL)] for i in range(nl)], pa.utf8())], names=["k", "a"])
    right = pa.RecordBatch.from_arrays([pa.array(rng.integers(0, 300, nr).astype(np.int32)), pa.array(rng.random(nr).astype(np.float32))], names=["rk", "b"])
    ld, rd = chq.DeviceRecordBatch.from_host(left, ctx), chq.DeviceRecordBatch.from_host(right, ctx)
    keys = [(A.ident("k"), A.ident("rk"))]
    joined = chq.join_records(ld, [[], []], rd, [[], []], keys, ctx=ctx, how="left")
    anti = chq.join_records(ld, [[], []], rd, [[], []], keys, ctx=ctx, how="anti").to_host()
    kept = chq.filter_record(joined, [[]] * 4, parse_expr("rk is null"), ctx=ctx).to_host()
    assert 0 < anti.num_rows < nl and kept.num_rows == anti.num_rows
    assert kept.column("rk").null_count == kept.num_rows and kept.column("b").null_count == kept.num_rows
    assert kept.column("k").to_pylist() == anti.column("k").to_pylist() and kept.column("a").to_pylist() == anti.column("a").to_pylist()
    rest = chq.filter_record(joined, [[]] * 4, parse_expr("rk is not null and a like '%a%'"), ctx=ctx).to_host()
    jh = joined.to_host()
    want = [(k, a) for k, a, rk in zip(jh.column("k").to_pylist(), jh.column("a").to_pylist(), jh.column("rk").to_pylist()) if rk is not None and "a" in a]
    assert list(zip(rest.column("k").to_pylist(), rest.column("a").to_pylist())) == want
