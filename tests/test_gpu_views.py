"""GPU: the calls of the engine on Arrow VIEWS -- what read_files and the group calls actually hand on: one upload cut into
`DeviceRecordBatch.slice` windows (Arrow offsets in the thousands, validity bitmaps with an unknown null count whose nulls
may lie outside the window), and the per-batch outputs of a device group call (slices of one dense buffer) fed into the
next call.  Every result is compared bit-exact with the CPU oracle run on the same rows as a host slice."""
import io

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

import chapterhouseqe_amd as chq
from chapterhouseqe_amd.sqlparse import parse_expr, parse_select
from oracle import oracle as O

from .cases import empty_aliases
from .helpers import batches_identical, explain_diff

pytestmark = pytest.mark.gpu

N = 70_000
CLEAN = (20_000, 26_000)   # rows in which no nullable column of a parent holds a null
# (offset, length) of the views of one group: every offset class of the bitmap (bit 0, inside a byte, byte / word / 64-row
# boundaries, past a 4 KiB page of rows, past 2^16), one window inside CLEAN; 2 rows at least, so the group keeps its
# one-launch paths
WINDOWS = [(0, 1500), (1, 1499), (7, 2000), (8, 64), (9, 1000), (63, 2), (64, 1700), (65, 777), (127, 1024), (4095, 1500),
           (4097, 999), (65_539, 2000), (CLEAN[0] + 3, 1800)]
# a group holding 0- and 1-row windows (the per-batch paths)
SHORT_WINDOWS = [(5, 0), (9, 1), (4097, 1), (64, 0), (130, 300), (65_539, 1), (CLEAN[0] + 1, 2)]
STAT_KEYS = ("rows_in", "rows_out", "tiles", "launches", "bytes_read_alg", "bytes_written_alg")

PRED_READ = ["x % 3 = 0 and f < 60.0", "flag = true or x > 600", "dec >= dec and f > 20.0"]   # the nullable, Boolean and 16-byte columns
PRED_COPY = ["f > 50.0", "id % 2 = 0"]                                                       # every column only copied
PROJECTION = "select id, x * 2 as x2, f + 1.0 as f1, flag, dec, ts, {strs} from t"


# ---- host parents ---------------------------------------------------------------------------------------------------------
def utf8_array(rng, lengths, valid, null_slot_bytes=False):
    """Utf8 from raw buffers: value i has lengths[i] bytes; a null slot holds its bytes too with `null_slot_bytes` (Arrow
    allows it, arrow-rs `nullif` produces it), else none (pyarrow's own form)"""
    lengths = np.asarray(lengths, np.int64)
    eff = lengths if null_slot_bytes else np.where(valid, lengths, 0)
    offs = np.zeros(len(lengths) + 1, np.int32)
    np.cumsum(eff, out=offs[1:])
    data = rng.integers(ord("a"), ord("z") + 1, int(offs[-1])).astype(np.uint8)
    nulls = int((~valid).sum())
    bitmap = pa.py_buffer(np.packbits(valid, bitorder="little").tobytes()) if nulls else None
    arr = pa.Array.from_buffers(pa.utf8(), len(lengths), [bitmap, pa.py_buffer(offs.tobytes()), pa.py_buffer(data.tobytes())],
                                null_count=nulls)
    arr.validate(full=True)
    return arr


def spread_mask(rng, n, share=0.15):
    """nulls over the whole parent except CLEAN"""
    m = rng.random(n) < share
    m[CLEAN[0]:CLEAN[1]] = False
    return m


def parent(seed, utf8, n=N):
    """id Int32, x Int32 (nulls), f Float32, flag Boolean (nulls), the Utf8 columns `utf8` names, dec Decimal128 (nulls),
    ts Timestamp(us).  Utf8 kinds: uL = one length L with nulls (null slots empty), kL = one length L without nulls,
    rag = 0..20 bytes with nulls, short = 1..6 bytes without nulls"""
    rng = np.random.default_rng(seed)
    cols = {"id": pa.array(rng.integers(-10**6, 10**6, n).astype(np.int32)),
            "x": pa.array(rng.integers(-1000, 1000, n).astype(np.int32), mask=spread_mask(rng, n)),
            "f": pa.array((rng.random(n) * 100).astype(np.float32)),
            "flag": pa.array(rng.random(n) < 0.5, mask=spread_mask(rng, n))}
    for name in utf8:
        if name == "rag":
            cols[name] = utf8_array(rng, rng.integers(0, 21, n), ~spread_mask(rng, n))
        elif name == "short":
            cols[name] = utf8_array(rng, rng.integers(1, 7, n), np.ones(n, bool))
        else:
            cols[name] = utf8_array(rng, np.full(n, int(name[1:])), ~spread_mask(rng, n) if name[0] == "u" else np.ones(n, bool))
    cols["dec"] = pa.array(rng.integers(-10**9, 10**9, n), mask=spread_mask(rng, n)).cast(pa.decimal128(24, 2))
    cols["ts"] = pa.array(rng.integers(0, 2**50, n), type=pa.timestamp("us"))
    return pa.RecordBatch.from_arrays(list(cols.values()), names=list(cols.keys()))


WIDE = ("u1", "u2", "u4", "u8", "u16", "rag", "short")   # more Utf8 columns than the fold serves: joined on the device
FOLD = {f"u{L}+short": (f"u{L}", "short") for L in (1, 2, 4, 8, 16)}   # two Utf8 columns: the one-launch fold
SCHEMAS = {"wide": WIDE, **FOLD, "u8+rag": ("u8", "rag"), "k4+k16": ("k4", "k16")}
_parents = {}


def host_parent(name):
    if name not in _parents:
        _parents[name] = parent(1000 + len(_parents), SCHEMAS[name])
    return _parents[name]


# ---- the view builder -----------------------------------------------------------------------------------------------------
def make_views(ctx, rec, windows):
    """`rec` uploaded once, unsliced, and cut into device views; returns [(view, expected host rows)].  Asserts that every
    view is the production shape: the offset it claims (over the parent's own) and an unknown null count wherever a bitmap
    rides along -- which it does for every column with nulls in the parent, whether the window holds any or not"""
    dev = chq.DeviceRecordBatch.from_host(rec, ctx)
    base = dev.describe_columns()
    out = []
    for off, ln in windows:
        v = dev.slice(off, ln)
        assert v.num_rows == ln
        for c, p, h in zip(v.describe_columns(), base, rec.columns):
            assert c["offset"] == p["offset"] + off and c["length"] == ln, (c["name"], off, c["offset"], p["offset"])
            if c["validity"]:
                assert c["null_count"] == -1, (c["name"], off, c["null_count"])
            if h.null_count:
                assert c["validity"], (c["name"], off)
        out.append((v, rec.slice(off, ln)))
    return out


def stats_of(ctx):
    s = ctx.last_stats()
    return {k: s[k] for k in STAT_KEYS}


def check_group_calls(c, views, sql, tag=""):
    """filter_records (device and host results, and through a RecordGroup) and filter_records_coalesced against the oracle
    per window; returns the stats of the device-result call"""
    al = empty_aliases(views[0][1])
    e = parse_expr(sql)
    devs = [v for v, _ in views]
    want = [O.filter_record(h, al, e) for _, h in views]
    got = chq.filter_records(devs, al, e, ctx=c)
    st = stats_of(c)
    for i, (g, w) in enumerate(zip(got, want)):
        gh = g.to_host()
        assert batches_identical(gh, w), f"{tag} {sql}: device result, window {i}:\n{explain_diff(gh, w)}"
    host = chq.filter_records(devs, al, e, ctx=c, device_result=False)
    for i, (g, w) in enumerate(zip(host, want)):
        assert batches_identical(g, w), f"{tag} {sql}: host result, window {i}:\n{explain_diff(g, w)}"
    grp = chq.RecordGroup(devs, c)
    again = chq.filter_records(grp, al, e, ctx=c, device_result=False)
    grp.release()
    for i, (g, w) in enumerate(zip(again, want)):
        assert batches_identical(g, w), f"{tag} {sql}: RecordGroup, window {i}"
    for dev_out in (True, False):
        big, per = chq.filter_records_coalesced(devs, al, e, ctx=c, device_result=dev_out)
        assert per == [w.num_rows for w in want], (tag, sql, per)
        bh = big.to_host() if dev_out else big
        assert bh.num_rows == sum(per)
        if bh.num_rows:
            whole = pa.Table.from_batches(want).combine_chunks().to_batches()[0]
            assert batches_identical(bh, whole, check_nullable=False), f"{tag} {sql}: coalesced ({dev_out}):\n{explain_diff(bh, whole)}"
    return st


def fresh_ctx(**opts):
    c = chq.Context(0)
    for k, v in opts.items():
        c.set_option(k, v)
    return c


@pytest.fixture(scope="module")
def ctx():
    c = chq.Context(0)
    yield c
    c.close()


# ---- group calls on views ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schema", list(SCHEMAS))
def test_group_calls_on_views(ctx, schema):
    rec = host_parent(schema)
    views = make_views(ctx, rec, WINDOWS)
    for sql in PRED_READ + PRED_COPY:
        check_group_calls(ctx, views, sql, schema)


@pytest.mark.parametrize("schema", ["wide", "u8+rag", "k4+k16"])
def test_group_calls_on_short_views(ctx, schema):
    """windows of 0 and 1 rows inside a group (the per-batch path serves such a group)"""
    views = make_views(ctx, host_parent(schema), SHORT_WINDOWS)
    for sql in ["x % 3 = 0 and f < 60.0", "f > 50.0"]:
        check_group_calls(ctx, views, sql, schema)


SWEEP = [{}, {"group_mode": 1}, {"group_mode": 2}, {"group_bits": 0}, {"group_fold": 0}, {"fold_utf8": 0},
         {"uniform_utf8_rows": 1}, {"uniform_utf8_rows": 0}, {"group_chunk_bytes": 1 << 30}, {"group_chunk_bytes": 20_000},
         {"tile_kind": -1}, {"tile_kind": 0}, {"tile_kind": 1}, {"split_rows": 512},
         {"group_mode": 2, "uniform_utf8_rows": 1}, {"group_mode": 1, "group_bits": 0, "tile_kind": 1},
         {"group_fold": 0, "fold_utf8": 0, "split_rows": 512}, {"group_chunk_bytes": 20_000, "uniform_utf8_rows": 1, "group_mode": 2},
         {"tile_kind": 0, "split_rows": 256, "group_mode": 1, "uniform_utf8_rows": 1}]


@pytest.mark.parametrize("opts", SWEEP, ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()) or "defaults")
def test_group_path_sweep_on_views(opts):
    """every path option against the defaults (plus a few combinations): a group with bitmapped strings (u8+rag: the fold and
    the bitmap compaction) and one of bitmap-free uniform strings (k4+k16: the uniform-length group path)"""
    c = fresh_ctx(**opts)
    for schema in ("u8+rag", "k4+k16"):
        views = make_views(c, host_parent(schema), WINDOWS)
        for sql in ["flag = true or x > 600", "id % 2 = 0"]:
            check_group_calls(c, views, sql, f"{schema} {opts}")
    c.close()


# ---- evidence that the paths ran -------------------------------------------------------------------------------------
def test_uniform_group_path_runs_on_views():
    """bitmap-free uniform strings in views take the uniform-length group path: its stats differ from the fold path's by
    exactly its offsets pass and its fixed-width reads (bytes_read_alg, group.cpp, uniform_group: (rows + batches) x 4 per column, L per
    row) against the fold's 8 per row and the kept bytes; the writes agree"""
    rec = host_parent("k4+k16")
    lens = [4, 16]
    st, co = {}, {}
    for u in (1, 0):
        c = fresh_ctx(uniform_utf8_rows=u, group_mode=2)   # (the nullable columns need the wave-packed form)
        views = make_views(c, rec, WINDOWS)
        for sql in ["id % 2 = 0", "flag = true or x > 600"]:
            st[(u, sql)] = check_group_calls(c, views, sql, f"uniform_utf8_rows={u}")
            chq.filter_records_coalesced([v for v, _ in views], empty_aliases(rec), parse_expr(sql), ctx=c)
            co[(u, sql)] = stats_of(c)
        c.close()
    rows, nb = sum(ln for _, ln in WINDOWS), len(WINDOWS)
    for sql in ["id % 2 = 0", "flag = true or x > 600"]:
        on, off = st[(1, sql)], st[(0, sql)]
        out = on["rows_out"]
        assert out == off["rows_out"] and on["rows_in"] == off["rows_in"] == rows
        assert on["bytes_written_alg"] == off["bytes_written_alg"], (sql, on, off)
        # the coalesced call counts the same writes: its offsets (rows_out + 1) x 4 per column like the fold's
        assert co[(1, sql)]["rows_out"] == out and co[(1, sql)]["bytes_written_alg"] == co[(0, sql)]["bytes_written_alg"], (sql, co)
        extra = sum((rows + nb) * 4 + rows * L - rows * 8 - out * L for L in lens)
        assert on["bytes_read_alg"] - off["bytes_read_alg"] == extra, (sql, on, off, extra)
        assert co[(1, sql)]["bytes_read_alg"] - co[(0, sql)]["bytes_read_alg"] == extra, (sql, co, extra)   # (the coalesced call ran it too)


def test_wave_packed_bitmap_path_runs_on_views():
    """a wave-packed group with bitmaps (group_mode 2, group_bits 1) is ONE filter launch plus one bit-compaction launch per
    joined bitmap (each Boolean column's values, each column's validity)"""
    rec = host_parent("u8+rag")
    c = fresh_ctx(group_mode=2)
    views = make_views(c, rec, WINDOWS)
    descs = [v.describe_columns() for v, _ in views]
    nbits = sum(f.type == pa.bool_() for f in rec.schema) + sum(any(d[i]["validity"] for d in descs) for i in range(rec.num_columns))
    for sql in ["flag = true or x > 600", "id % 2 = 0"]:
        st = check_group_calls(c, views, sql, "wave-packed")
        assert st["launches"] == 1 + nbits, (sql, st, nbits)
        assert st["rows_in"] == sum(ln for _, ln in WINDOWS)
    c.close()


# ---- single-batch entry points on the same views -----------------------------------------------------------------------
@pytest.mark.parametrize("opts", [{}, {"split_rows": 512}, {"tile_kind": 0}, {"uniform_utf8_rows": 1}],
                         ids=["defaults", "split_rows=512", "tile_kind=0", "uniform_utf8_rows=1"])
@pytest.mark.parametrize("schema", ["wide", "k4+k16"])
def test_single_batch_calls_on_views(schema, opts):
    c = fresh_ctx(**opts)
    rec = host_parent(schema)
    windows = WINDOWS + [w for w in SHORT_WINDOWS if w[1] < 2]
    views = make_views(c, rec, windows)
    al = empty_aliases(rec)
    strs = ", ".join(SCHEMAS[schema])
    fields = parse_select(PROJECTION.format(strs=strs)).projection
    for (v, h), w in zip(views, windows):
        tag = (schema, opts, w)
        for sql in ["x % 3 = 0 and f < 60.0", "dec >= dec and f > 20.0", "f > 50.0"]:
            e = parse_expr(sql)
            want = O.filter_record(h, al, e)
            got = chq.filter_record(v, al, e, ctx=c).to_host()
            assert batches_identical(got, want), f"{tag} {sql}:\n{explain_diff(got, want)}"
            wantp = O.project_record(fields, want, al)
            for fuse in (0, 1, 2):
                c.set_option("fuse", fuse)
                gp = chq.filter_project_record(e, fields, v, al, ctx=c).to_host()
                assert batches_identical(gp, wantp, nan_payload=False), f"{tag} {sql} fuse={fuse}:\n{explain_diff(gp, wantp)}"
            c.set_option("fuse", 1)
        gp = chq.project_record(fields, v, al, ctx=c).to_host()
        wp = O.project_record(fields, h, al)
        assert batches_identical(gp, wp, nan_payload=False), f"{tag} projection:\n{explain_diff(gp, wp)}"
    c.close()


# ---- chained calls: FilterTask -> MaterializeFilesTask -------------------------------------------------------------------
CHAIN_COLS = ["id", "x", "f", "flag", "u8", "rag"]   # the types the Parquet writer takes


@pytest.fixture(scope="module")
def chain():
    """the device outputs of one group call over views (slices of one dense buffer: large offsets, null counts -1) next to
    the same step on the host"""
    c = chq.Context(0)
    full = host_parent("u8+rag")
    rec = full.select(CHAIN_COLS)
    views = make_views(c, rec, WINDOWS)
    al = empty_aliases(rec)
    e = parse_expr("x % 3 <> 0 or f < 30.0")
    outs = chq.filter_records([v for v, _ in views], al, e, ctx=c)
    want = [O.filter_record(h, al, e) for _, h in views]
    offsets, unknown = [], 0
    for o, w in zip(outs, want):
        assert o.num_rows == w.num_rows
        for d in o.describe_columns():
            offsets.append(d["offset"])
            if d["validity"]:
                assert d["null_count"] == -1, d
                unknown += 1
    assert max(offsets) > 1000 and unknown > 0, (max(offsets), unknown)   # the shape production hands on
    yield c, outs, want, al
    c.close()


def test_chain_filter_then_filter(chain):
    c, outs, want, al = chain
    for sql in ["flag = true or x > 600", "f > 50.0"]:
        e = parse_expr(sql)
        exp = [O.filter_record(w, al, e) for w in want]
        got = chq.filter_records(outs, al, e, ctx=c)
        for i, (g, x) in enumerate(zip(got, exp)):
            gh = g.to_host()
            assert batches_identical(gh, x), f"{sql}, output {i}:\n{explain_diff(gh, x)}"
        big, per = chq.filter_records_coalesced(outs, al, e, ctx=c)
        assert per == [x.num_rows for x in exp]
        if big.num_rows:
            whole = pa.Table.from_batches(exp).combine_chunks().to_batches()[0]
            assert batches_identical(big.to_host(), whole, check_nullable=False), sql


def test_chain_filter_then_project(chain):
    c, outs, want, al = chain
    fields = parse_select("select id, x * 2 as x2, f + 1.0 as f1, flag, u8, rag from t").projection
    for i, (o, w) in enumerate(zip(outs, want)):
        got = chq.project_record(fields, o, al, ctx=c).to_host()
        exp = O.project_record(fields, w, al)
        assert batches_identical(got, exp, nan_payload=False), f"output {i}:\n{explain_diff(got, exp)}"


def test_chain_filter_then_parquet(chain):
    c, outs, want, al = chain
    data = chq.records_to_parquet(outs, ctx=c)
    f = pq.ParquetFile(io.BytesIO(data))
    assert f.metadata.num_row_groups == len(want)
    for i, w in enumerate(want):
        got = f.read_row_group(i)
        got = got.combine_chunks().to_batches()[0] if got.num_rows else w.slice(0, 0)
        assert batches_identical(got, w, check_nullable=False), f"row group {i}:\n{explain_diff(got, w)}"
        rg = f.metadata.row_group(i)
        assert rg.num_rows == w.num_rows
        for j in range(w.num_columns):
            st = rg.column(j).statistics
            assert st is not None and st.has_null_count and st.null_count == w.column(j).null_count, (i, w.schema.field(j).name, st)


def test_chain_filter_then_ipc(chain):
    c, outs, want, al = chain
    for i, (o, w) in enumerate(zip(outs, want)):
        msg = chq.record_to_ipc(o, ctx=c).to_bytes()
        back = chq.record_from_ipc(msg, ctx=c).to_host()
        assert batches_identical(back, w), f"output {i}:\n{explain_diff(back, w)}"
        host = pa.ipc.open_stream(msg).read_next_batch()
        assert batches_identical(host, w), f"output {i} (pyarrow reader):\n{explain_diff(host, w)}"


# ---- named regressions ------------------------------------------------------------------------------------------------
# views of one length, as tasks.py cuts row groups: the group is wave-packed by default, which the bitmapped paths need
REG_WINDOWS = [(off, 2000) for off in (8, 9, 63, 64, 65, 127, 4095, 4097, CLEAN[0] + 3, 65_539)]


def test_uniform_utf8_with_bitmap_in_views_keeps_its_nulls():
    """regression: a uniform-length Utf8 column with a bitmap (nulls only in rows 0..7 and past every window) in views at
    offsets >= 8.  The uniform-length group path used to read such a column's validity from bit 0 instead of the view's
    offset: nulls appeared in the output.  Such a column now keeps the string path -- same stats as with the path off"""
    rng = np.random.default_rng(41)
    base = host_parent("u8+rag")
    valid = np.ones(N, bool)
    valid[:8] = False
    valid[69_000:] = rng.random(N - 69_000) < 0.5
    cols = dict(zip(base.schema.names, base.columns))
    cols["u8"] = utf8_array(rng, np.full(N, 8), valid)
    cols["k8"] = utf8_array(rng, np.full(N, 8), np.ones(N, bool))
    del cols["rag"]
    rec = pa.RecordBatch.from_arrays(list(cols.values()), names=list(cols.keys()))
    for mode in (0, 2):
        st = {}
        for u in (1, 0):
            c = fresh_ctx(uniform_utf8_rows=u, group_mode=mode)
            views = make_views(c, rec, REG_WINDOWS)
            for sql in ["id = id", "id % 2 = 0", "f > 25.0"]:
                st[(u, sql)] = check_group_calls(c, views, sql, f"group_mode={mode} uniform_utf8_rows={u}")
            c.close()
        for sql in ["id = id", "id % 2 = 0", "f > 25.0"]:
            assert st[(1, sql)] == st[(0, sql)], (mode, sql, st[(1, sql)], st[(0, sql)])


@pytest.mark.parametrize("shape", ["whole", "host-sliced", "views"])
def test_utf8_null_slots_holding_bytes_coalesced(shape):
    """regression: a Utf8 column whose null slots hold L bytes each passes the uniform-length check; the coalesced form of the
    uniform-length group path rebuilt the column without its validity, so those nulls came back as values"""
    rng = np.random.default_rng(43)
    n = 6000
    c = fresh_ctx(uniform_utf8_rows=1)
    if shape == "views":
        base = host_parent("u8+rag").slice(0, N)
        valid = ~spread_mask(rng, N, 0.2)
        cols = dict(zip(base.schema.names, base.columns))
        cols["u8"] = utf8_array(rng, np.full(N, 8), valid, null_slot_bytes=True)
        del cols["rag"]
        rec = pa.RecordBatch.from_arrays(list(cols.values()), names=list(cols.keys()))
        views = make_views(c, rec, REG_WINDOWS)
    else:
        views = []
        for i in range(8):
            r = np.random.default_rng(500 + i)
            valid = r.random(n) < 0.8
            rec = pa.record_batch({"id": pa.array(r.integers(0, 1000, n).astype(np.int32)),
                                   "s": utf8_array(r, np.full(n, 8), valid, null_slot_bytes=True),
                                   "f": pa.array((r.random(n) * 100).astype(np.float32))})
            if shape == "host-sliced":
                rec = rec.slice(1 + 7 * i, n - 100)
            views.append((chq.DeviceRecordBatch.from_host(rec, c), rec))
    for sql in ["id % 2 = 0", "f > 25.0"]:
        check_group_calls(c, views, sql, shape)
    c.close()
