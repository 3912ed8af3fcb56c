"""GPU: the scalar string functions on the device (strfn.hip) -- `||`, upper / lower, length, octet_length, substring, trim.
Every result is compared buffer by buffer (offsets, bytes, validity, null count, or the Int32 values) with
tests/strfn_reference.py, which the CPU tier pins to sqlite3 and pyarrow.compute.  Columns are built from raw buffers, so that
rows of invalid UTF-8 and null slots that enclose bytes can be fed in; results are read back as binary."""
import os
import re

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest

import chapterhouseqe_amd as chq
from chapterhouseqe_amd.sqlparse import parse_expr, parse_select
from oracle import oracle as O

from . import strfn_reference as R
from .cases import empty_aliases
from .helpers import batches_identical, explain_diff

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_HDR = open(os.path.join(ROOT, "chapterhouseqe_amd", "csrc", "strfn_device.h")).read()
WAVE_MODE_BYTES = int(re.search(r"STRFN_WAVE_MODE_BYTES\s*=\s*(\d+)", _HDR).group(1))
MAX_PARTS = int(re.search(r"STRFN_MAX_PARTS\s*=\s*(\d+)", _HDR).group(1))
GRID_ROWS = 256 * 32 * 256          # rows one pass of the rows / gather grid covers (strfn.hip: the cap of rows_grid)
GRID_MAP_BYTES = 256 * 16 * 256 * 16  # bytes one pass of the byte map's grid covers


@pytest.fixture(scope="module")
def ctx():
    c = chq.Context(0)
    yield c
    c.close()


# ---- columns from raw buffers -------------------------------------------------------------------------------------------------
GARBAGE = [b"\xff\xfe", b"  Ab  ", b"\x80\x80ab", b"", b"zz" * 20]


def utf8_column(cells, lead=b""):
    """cells: bytes, or None = a null slot, which encloses some of GARBAGE; `lead`: bytes in front of row 0 (offsets[0] != 0)"""
    blobs = [GARBAGE[i % len(GARBAGE)] if c is None else c for i, c in enumerate(cells)]
    offs = np.zeros(len(cells) + 1, np.int64)
    np.cumsum([len(b) for b in blobs], out=offs[1:])
    offs += len(lead)
    valid = np.array([c is not None for c in cells], bool)
    nulls = int((~valid).sum())
    bitmap = pa.py_buffer(np.packbits(valid, bitorder="little").tobytes()) if nulls else None
    return pa.Array.from_buffers(pa.utf8(), len(cells), [bitmap, pa.py_buffer(offs.astype(np.int32).tobytes()), pa.py_buffer(lead + b"".join(blobs))], null_count=nulls)


def batch(s_cells, t_cells=None, seed=0):
    """s, t Utf8 (t: the cells of s rotated, nulls in other rows, unless given), id Int32 with nulls"""
    n = len(s_cells)
    if t_cells is None:
        t_cells = [None if i % 7 == 2 else (s_cells[(i + 3) % n] or b"Tt") for i in range(n)]
    rng = np.random.default_rng(seed)
    return pa.RecordBatch.from_arrays([utf8_column(s_cells), utf8_column(t_cells), pa.array(np.arange(n, dtype=np.int32), mask=(rng.random(n) < 0.2) if n else None)],
                                      names=["s", "t", "id"])


def cells_of(arr):
    return arr.view(pa.binary()).to_pylist()


def raw_cells(arr):
    """the bytes every slot encloses, null slots included"""
    n = len(arr)
    offs = np.frombuffer(arr.buffers()[1], np.int32, n + 1, arr.offset * 4)
    data = arr.buffers()[2].to_pybytes() if arr.buffers()[2] is not None else b""
    return [data[offs[i]:offs[i + 1]] for i in range(n)]


def with_nulls(cells, nulls, step=5):
    return [None if nulls and i % step == 2 else c for i, c in enumerate(cells)]


# ---- comparing a result -------------------------------------------------------------------------------------------------------
def check_array(arr, want, what, null_bytes=None):
    """`arr` (a host array read back) against `want`: a list of bytes / int / None.  `null_bytes`: what the null slots of a Utf8
    result enclose -- nothing, except behind the byte map (upper / lower of a column), which keeps the input's offsets and maps
    the bytes of null rows like any others"""
    n = len(want)
    assert len(arr) == n and arr.offset == 0, what
    nulls = sum(w is None for w in want)
    assert arr.null_count == nulls, (what, arr.null_count, nulls)
    if nulls:
        assert arr.is_valid().to_pylist() == [w is not None for w in want], what
    else:
        assert arr.buffers()[0] is None, what
    if any(isinstance(w, int) for w in want) or (arr.type == pa.int32()):
        assert arr.type == pa.int32(), (what, arr.type)
        got = arr.to_pylist()
        bad = [i for i in range(n) if got[i] != want[i]][:8]
        assert not bad, f"{what}: first differences at {bad}: {[(got[i], want[i]) for i in bad]}"
        return
    assert arr.type == pa.utf8(), (what, arr.type)
    if n == 0:
        return
    exp_offs = np.zeros(n + 1, np.int64)
    if null_bytes is not None:
        want = [null_bytes[i] if w is None else w for i, w in enumerate(want)]
    np.cumsum([0 if w is None else len(w) for w in want], out=exp_offs[1:])
    offs = np.frombuffer(arr.buffers()[1], np.int32, n + 1)
    if not np.array_equal(offs, exp_offs):
        bad = np.flatnonzero(offs != exp_offs)[:8]
        raise AssertionError(f"{what}: offsets differ first at {bad.tolist()}: got {offs[bad].tolist()} expected {exp_offs[bad].tolist()}")
    total = int(exp_offs[-1])
    data = arr.buffers()[2].to_pybytes()[:total] if total else b""
    exp = b"".join(w for w in want if w is not None)
    if data != exp:
        at = next(i for i in range(total) if data[i:i + 1] != exp[i:i + 1])
        row = int(np.searchsorted(exp_offs, at, side="right")) - 1
        raise AssertionError(f"{what}: byte {at} (row {row}, place {at - int(exp_offs[row])}): got {data[at:at + 8]!r} expected {exp[at:at + 8]!r}")


BYTE_MAPS = {"upper(s)": ("s", R.upper), "lower(s)": ("s", R.lower), "upper(t)": ("t", R.upper), "lower(t)": ("t", R.lower)}


def null_bytes_of(host, sql):
    if sql not in BYTE_MAPS:
        return None
    col, f = BYTE_MAPS[sql]
    return [f(b) for b in raw_cells(host.column(col))]


def check_value(c, rec, host, sql, want, what):
    arr, is_scalar = chq.compute_value(rec, empty_aliases(host), parse_expr(sql), ctx=c)
    assert not is_scalar, (what, sql)
    check_array(arr, want, f"{what}: {sql}", null_bytes_of(host, sql))


# ---- the forms ------------------------------------------------------------------------------------------------------------------
def un(f, *args):
    return lambda s, t: None if s is None else f(s, *args)


def bi(f):
    return lambda s, t: None if s is None or t is None else f(s, t)


FORMS = [
    ("upper(s)", un(R.upper)), ("lower(s)", un(R.lower)), ("LENGTH(s)", un(R.length)), ("char_length(s)", un(R.length)), ("octet_length(s)", un(R.octet_length)),
    ("trim(s)", un(R.trim)), ("ltrim(s)", un(R.ltrim)), ("rtrim(s)", un(R.rtrim)),
    ("substring(s from 2 for 3)", un(R.substring, 2, 3)), ("substring(s from 1)", un(R.substring, 1)), ("substr(s, 0, 2)", un(R.substring, 0, 2)),
    ("substring(s from -3 for 5)", un(R.substring, -3, 5)), ("substring(s, 3)", un(R.substring, 3)), ("substring(s from 1 for 0)", un(R.substring, 1, 0)),
    ("s || t", bi(lambda s, t: s + t)), ("s || '-' || t", bi(lambda s, t: s + b"-" + t)), ("'<' || s || '>'", un(lambda s: b"<" + s + b">")),
    ("s || ''", un(lambda s: s)), ("upper(s) || lower(t)", bi(lambda s, t: R.upper(s) + R.lower(t))), ("length(s || t)", bi(lambda s, t: R.length(s + t))),
    ("upper(trim(s))", un(lambda s: R.upper(R.trim(s)))), ("length(substring(s from 2))", un(lambda s: R.length(R.substring(s, 2)))),
]
SHORT_FORMS = [FORMS[i] for i in (0, 2, 5, 8, 15)]


def check_forms(c, rec, host, forms, what):
    s, t = cells_of(host.column("s")), cells_of(host.column("t"))
    for sql, f in forms:
        check_value(c, rec, host, sql, [f(a, b) for a, b in zip(s, t)], what)


def check_projection(c, rec, host, what):
    """a computed Utf8 item and a computed Int32 item (and more) in ONE SELECT: names, types, and nullable iff a null is held"""
    s, t = cells_of(host.column("s")), cells_of(host.column("t"))
    sel = parse_select("select upper(s) as u, length(s) as n, s || '-' || t as c, id, octet_length(t), substring(s from 2 for 2) from x")
    out = chq.project_record(sel.projection, rec, empty_aliases(host), ctx=c, device_result=False)
    assert out.schema.names == ["u", "n", "c", "id", "unnamed_1", "unnamed_2"], (what, out.schema.names)   # (the unnamed items are counted)
    wants = [[None if a is None else R.upper(a) for a in s], [None if a is None else R.length(a) for a in s],
             [None if a is None or b is None else a + b"-" + b for a, b in zip(s, t)], None, [None if b is None else len(b) for b in t],
             [None if a is None else R.substring(a, 2, 2) for a in s]]
    for k, want in enumerate(wants):
        if want is None:
            continue
        check_array(out.column(k), want, f"{what}: select item {k}", null_bytes_of(host, "upper(s)") if k == 0 else None)
        assert out.schema.field(k).nullable == any(w is None for w in want), (what, k)
    assert [out.schema.field(k).type for k in (0, 1, 2, 4, 5)] == [pa.utf8(), pa.int32(), pa.utf8(), pa.int32(), pa.utf8()]


POOL = [b"", b"a", b"Ab", b" aB ", b"  ", b"h\xc3\xa9llo", b"\xe6\x97\xa5\xe6\x9c\xac\xe8\xaa\x9e", b"a\xf0\x9f\x98\x80\xc3\xa9 ", b"zZ@[`{", b"x" * 17, b" q", b"q ",
        b"Hello, World", b"\xc3\x80\xc3\x89bc", b"   pad   ", b"MiXeD cAsE 123"]


def pool_cells(n, nulls, seed):
    rng = np.random.default_rng(seed)
    cells = [POOL[(i * 7 + seed) % len(POOL)] for i in range(n)]
    if nulls:
        cells = [None if rng.random() < 0.3 else v for v in cells]
        if n:
            cells[n // 2] = None
    return cells


# ---- row counts of one wave, one block and more; null slots enclose garbage ----------------------------------------------------
@pytest.mark.parametrize("nulls", [False, True], ids=["dense", "nulls"])
@pytest.mark.parametrize("rows", [0, 1, 63, 64, 65, 257])
def test_row_counts(ctx, rows, nulls):
    host = batch(pool_cells(rows, nulls, rows + 1), seed=rows)
    dev = chq.DeviceRecordBatch.from_host(host, ctx)
    check_forms(ctx, dev, host, FORMS, f"{rows} rows")
    check_forms(ctx, host, host, SHORT_FORMS, f"{rows} rows, host record")
    if rows:
        check_projection(ctx, dev, host, f"{rows} rows")
        check_projection(ctx, host, host, f"{rows} rows, host record")


@pytest.mark.parametrize("nulls", [False, True], ids=["dense", "nulls"])
@pytest.mark.parametrize("rows", [1, 64, 100])
def test_all_empty_column_without_a_data_buffer(ctx, rows, nulls):
    valid = np.arange(rows + 1) % 3 != 1
    ids = pa.RecordBatch.from_arrays([pa.array(np.zeros(rows + 1, np.int32)), pa.array(np.arange(rows + 1, dtype=np.int32)), pa.array(valid)], names=["o", "id", "v"])
    up = chq.DeviceRecordBatch.from_host(ids, ctx)
    s_desc = {"name": "s", "format": "u", "values": up.column_buffer_address(0)}
    if nulls:
        s_desc.update(validity=up.column_buffer_address(2), null_count=int((~valid[:rows]).sum()), nullable=True)
    dev = chq.DeviceRecordBatch.from_device_buffers([s_desc, dict(s_desc, name="t"), {"name": "id", "format": "i", "values": up.column_buffer_address(1)}], rows, ctx, keepalive=[up])
    assert dev.column_buffer_address(0, 2) == 0
    cells = [(b"" if ok or not nulls else None) for ok in valid[:rows]]
    host = pa.RecordBatch.from_arrays([pa.array(cells, pa.binary()).view(pa.utf8())] * 2 + [ids.column(1).slice(0, rows)], names=["s", "t", "id"])
    check_forms(ctx, dev, host, FORMS, "no data buffer")


# ---- sliced device views --------------------------------------------------------------------------------------------------------
def test_sliced_device_views(ctx):
    """offsets[0] != 0 at every residue mod 16 (the byte map's head), validity bit offsets that are no multiple of 8, windows
    whose byte range ends 1..15 bytes before the parent's"""
    n = 300
    rng = np.random.default_rng(12)
    cells = [bytes((65 + (i * 5 + j) % 58) for j in range(int(rng.integers(0, 40)))) for i in range(n)]
    for i in range(0, 40):
        cells[i] = bytes(97 + (i + j) % 26 for j in range(1 + i % 3))       # short rows first: the residues come by quickly
    cells = with_nulls(cells, True, 9)
    for i in range(120, 160):                                              # a stretch without nulls
        cells[i] = cells[i] or b"Stretch"
    for k in range(1, 16):                                                 # the last 15 rows: 1 byte each, so a window that stops k
        cells[n - k] = bytes([96 + k])                                     # rows short of the end stops k bytes short of it
    host = batch(cells, seed=3)
    dev = chq.DeviceRecordBatch.from_host(host, ctx)
    offs = np.frombuffer(host.column("s").buffers()[1], np.int32, n + 1)
    first_with = {}
    for i in range(1, 200):
        first_with.setdefault(int(offs[i]) % 16, i)
    assert len(first_with) == 16, sorted(first_with)
    windows = [(i, 37 + r) for r, i in sorted(first_with.items())] + [(1, 299), (7, 64), (9, 65), (63, 2), (64, 64), (77, 0), (129, 171), (120, 40)]
    windows += [(200 + k, n - k - (200 + k)) for k in range(1, 16)]
    assert any(o % 8 for o, _ in windows)
    for off, ln in windows:
        check_forms(ctx, dev.slice(off, ln), host.slice(off, ln), SHORT_FORMS + [FORMS[1], FORMS[15]], f"device view ({off}, {ln})")
    for off, ln in windows[3::7]:
        check_forms(ctx, host.slice(off, ln), host.slice(off, ln), SHORT_FORMS, f"host slice ({off}, {ln})")
    inner = dev.slice(120, 40)           # a bitmap rides along, no null inside: the result is not nullable
    out = chq.project_record(parse_select("select upper(s) as u, length(s) as n, trim(s) as w from x").projection, inner, empty_aliases(host), ctx=ctx, device_result=False)
    assert [f.nullable for f in out.schema] == [False, False, False]


@pytest.mark.parametrize("total", [0, 1, 15, 16, 17, 31, 33])
def test_byte_map_total_lengths(ctx, total):
    """the whole byte range of the column: shorter than one 16-byte access, exactly one, one and ragged ends"""
    body = bytes(65 + (j * 7) % 58 for j in range(total))
    for cells in ([body], [body[:total // 2], body[total // 2:]], [b"", body, b""]):
        host = batch(cells, t_cells=[b"t"] * len(cells))
        check_forms(ctx, chq.DeviceRecordBatch.from_host(host, ctx), host, FORMS[:2], f"{total} bytes in {len(cells)} rows")


def test_byte_map_alignment_phases(ctx):
    """a body of whole 16-byte accesses with ragged ends, at every alignment phase of the input against the output (whose
    byte 0 is the view's first byte): the view starts 0..15 bytes into the parent's data"""
    for phase in range(16):
        for tail in (0, 1, 15):
            cells = [bytes(97 + j % 26 for j in range(phase))] + [bytes(65 + (i * 3 + j) % 58 for j in range(29)) for i in range(7)] + [b"Q" * tail, b"end"]
            host = batch(cells, t_cells=[b"t"] * len(cells))
            dev = chq.DeviceRecordBatch.from_host(host, ctx)
            check_forms(ctx, dev.slice(1, len(cells) - 2), host.slice(1, len(cells) - 2), FORMS[:2], f"phase {phase}, tail {tail}")


# ---- row lengths in every lane position -------------------------------------------------------------------------------------------
CYCLE = [0, 1, 3, 4, 5, 15, 16, 17, 63, 64, 65]


def named_row(i, length):
    """bytes that name their row and their place in it: letters of both cases, a space now and then at the ends"""
    body = bytearray((65 if (i + j) % 2 else 97) + (i * 3 + j) % 26 for j in range(length))
    if length and i % 4 == 1:
        body[0] = 0x20
    if length > 1 and i % 4 == 2:
        body[-1] = 0x20
    return bytes(body)


@pytest.mark.parametrize("nulls", [False, True], ids=["dense", "nulls"])
def test_row_lengths_in_every_lane_position(ctx, nulls):
    """the lengths 0 .. 65 cycle through the rows; 11 and 64 are coprime, so over 704 rows every length meets every lane"""
    n = 64 * len(CYCLE)
    cells = with_nulls([named_row(i, CYCLE[i % len(CYCLE)]) for i in range(n)], nulls, 13)
    host = batch(cells, seed=5)
    check_forms(ctx, chq.DeviceRecordBatch.from_host(host, ctx), host, FORMS, "cycle")


# ---- lane per row / wave per row ------------------------------------------------------------------------------------------------------
WAVE_FORMS = FORMS + [("substring(s from 60 for 10)", un(R.substring, 60, 10)), ("substring(s from 64)", un(R.substring, 64)), ("substring(s from 65 for 64)", un(R.substring, 65, 64)),
                      ("substring(s from 128 for 2)", un(R.substring, 128, 2)), ("substring(s from 2 for 4000)", un(R.substring, 2, 4000)),
                      ("substring(s from 0 for 64)", un(R.substring, 0, 64))]


def wide_row(i, length):
    """multi-byte code points among letters and spaces, so that starts and step boundaries do not coincide"""
    unit = [b"a", b"B", b"\xc3\xa9", b" ", b"\xe6\x97\xa5", b"z", b"\xf0\x9f\x98\x80", b"Q"]
    out = b""
    k = i
    while len(out) < length:
        piece = unit[k % len(unit)]
        out += piece if len(out) + len(piece) <= length else b"x" * (length - len(out))
        k += 3
    return out


@pytest.mark.parametrize("nulls", [False, True], ids=["dense", "nulls"])
def test_wave_mode_threshold(ctx, nulls):
    """64 rows holding exactly the threshold (lane per row), one byte more (wave per row), and much more; then the same
    rows behind a wave of short ones and in front of a partial wave -- the mode is per wave"""
    per = WAVE_MODE_BYTES // 64
    rows = [wide_row(i, per) for i in range(64)]
    rows[-1] += b"a" * (WAVE_MODE_BYTES - 64 * per)
    for extra, what in ((0, "at the threshold"), (1, "one byte over"), (WAVE_MODE_BYTES, "far over")):
        cells = list(rows)
        cells[17] = cells[17] + b"b" * extra
        assert sum(len(v) for v in cells) == WAVE_MODE_BYTES + extra
        host = batch(with_nulls(cells, nulls, 7), seed=6)
        check_forms(ctx, chq.DeviceRecordBatch.from_host(host, ctx), host, WAVE_FORMS, what)
    many = [POOL[i % len(POOL)] for i in range(64)] + rows[:17] + [rows[17] + b"b"] + rows[18:] + rows[1:40]
    host = batch(with_nulls(many, nulls, 9), seed=8)
    dev = chq.DeviceRecordBatch.from_host(host, ctx)
    check_forms(ctx, dev, host, WAVE_FORMS, "three waves")
    check_forms(ctx, dev.slice(5, 150), host.slice(5, 150), SHORT_FORMS, "three waves, view")


@pytest.mark.parametrize("nulls", [False, True], ids=["dense", "nulls"])
def test_wave_mode_step_boundaries(ctx, nulls):
    """wave per row: rows of 63 .. 129 bytes, spaces that fill whole steps, one row of 5 000 bytes among empties"""
    filler = wide_row(1, WAVE_MODE_BYTES + 1)
    cells = [filler] + [wide_row(i, ln) for i, ln in enumerate([63, 64, 65, 127, 128, 129])] + [named_row(i, ln) for i, ln in enumerate([63, 64, 65, 127, 128, 129])]
    cells += [b" " * 63 + b"a", b" " * 64 + b"a", b"a" + b" " * 63, b"a" + b" " * 64, b" " * 64, b" " * 129, b" " * 70 + b"Mid dle" + b" " * 70, b"\x80" * 70 + b"a" + b"\xbf" * 70]
    cells += [POOL[i % len(POOL)] for i in range(64 - len(cells))]
    assert len(cells) == 64
    host = batch(with_nulls(cells, nulls, 7), seed=2)
    check_forms(ctx, chq.DeviceRecordBatch.from_host(host, ctx), host, WAVE_FORMS, "step boundaries")
    lone = [b""] * 64
    lone[41] = wide_row(2, 5000)
    host = batch(lone, t_cells=[b""] * 20 + [named_row(3, 4200)] + [b""] * 43, seed=2)
    check_forms(ctx, chq.DeviceRecordBatch.from_host(host, ctx), host, WAVE_FORMS, "one long row among empties")


# ---- substring windows ---------------------------------------------------------------------------------------------------------------
def test_substring_windows(ctx):
    """window edges on, before and after 2-, 3- and 4-byte code points; p in {-3, 0, 1, 2, length, length + 1}; n absent, 0, 1
    and past the end; rows of invalid UTF-8"""
    valid_rows = [s.encode() for s in ["", "a", "é", "日", "😀", "aé", "éa", "a日b", "日a日", "😀a", "a😀", "é日😀", "😀日é", "abc", "ab😀cd", "  é  "]]
    cells = valid_rows + R.INVALID + [None, b"tail"]
    host = batch(cells, seed=4)
    dev = chq.DeviceRecordBatch.from_host(host, ctx)
    lengths = sorted({R.length(c) for c in valid_rows})
    positions = sorted({-3, 0, 1, 2} | set(lengths) | {n + 1 for n in lengths})
    forms = []
    for p in positions:
        for n in (None, 0, 1, 2, 100):
            forms.append((R.substring_sql("s", p, n, comma=(p + (n or 0)) % 2 == 0), un(R.substring, p, n)))
    forms += [("substr(s, 2, 2147483647)", un(R.substring, 2, 2147483647)), ("substring(s from -2147483648 for 2147483647)", un(R.substring, -2147483648, 2147483647)),
              ("substring(s from 2147483647)", un(R.substring, 2147483647)), ("substring(s from (2) for (1))", un(R.substring, 2, 1))]
    check_forms(ctx, dev, host, forms, "windows")
    check_forms(ctx, dev, host, FORMS, "invalid rows, every function")
    check_forms(ctx, host, host, forms[::6], "windows, host record")


def test_trim_shapes(ctx):
    cells = [b"", b" ", b"  ", b" " * 17, b" " * 63, b"a", b"ab", b"a b", b"a  b  c", b" a", b"a ", b"  a b  ", b"\ta\t", b" \t ", b"\xc3\xa9 ", b" \xc3\xa9", None, b"   x", b"x   "] * 4
    host = batch(cells, seed=1)
    check_forms(ctx, chq.DeviceRecordBatch.from_host(host, ctx), host, FORMS[5:8] + [("trim(s) || '|'", un(lambda s: R.trim(s) + b"|")), ("length(rtrim(s))", un(lambda s: R.length(R.rtrim(s))))], "trim")


# ---- || ---------------------------------------------------------------------------------------------------------------------------
def test_concat_parts(ctx):
    """2, 3 and 8 parts in one operation, 9 and 17 nested; literals between columns, the empty literal, nulls of the parts in
    different rows, a part that is itself a function"""
    host = batch(pool_cells(130, True, 3), seed=9)
    dev = chq.DeviceRecordBatch.from_host(host, ctx)
    s, t = cells_of(host.column("s")), cells_of(host.column("t"))
    assert any(a is None and b is not None for a, b in zip(s, t)) and any(b is None and a is not None for a, b in zip(s, t))

    def chain(k):
        names = ["s" if i % 2 == 0 else "t" for i in range(k)]
        return " || ".join(names), bi(lambda a, b: b"".join(a if nm == "s" else b for nm in names))
    forms = [chain(2), chain(3), chain(MAX_PARTS), chain(MAX_PARTS + 1), chain(2 * MAX_PARTS + 1),
             ("s || '-' || t", bi(lambda a, b: a + b"-" + b)), ("s || '' || t || ''", bi(lambda a, b: a + b)), ("'' || s", un(lambda a: a)),
             ("'[' || s || '|' || s || ']'", un(lambda a: b"[" + a + b"|" + a + b"]")), ("(s || t) || (t || s)", bi(lambda a, b: a + b + b + a)),
             ("upper(s) || '/' || lower(s) || '/' || trim(t)", bi(lambda a, b: R.upper(a) + b"/" + R.lower(a) + b"/" + R.trim(b))),
             ("s || substring(t from 2 for 2)", bi(lambda a, b: a + R.substring(b, 2, 2))), ("upper(s || t)", bi(lambda a, b: R.upper(a + b))),
             ("'é' || s || '日本'", un(lambda a: "é".encode() + a + "日本".encode()))]
    check_forms(ctx, dev, host, forms, "||")
    check_forms(ctx, host, host, forms[::3], "||, host record")
    check_forms(ctx, dev.slice(3, 100), host.slice(3, 100), forms[:6], "||, view")


def test_concat_of_parts_sliced_differently(ctx):
    """the two operands are views at different row offsets of their own buffers"""
    n = 90
    parent = batch(pool_cells(n + 20, True, 5), seed=2)
    up = chq.DeviceRecordBatch.from_host(parent, ctx)
    cols = up.describe_columns()
    for c, off in zip(cols, (3, 11, 5)):
        c["offset"] += off
        if c["validity"] and c["null_count"] != 0:
            c["null_count"] = -1
    dev = chq.DeviceRecordBatch.from_device_buffers(cols, n, ctx=ctx, keepalive=[up])
    host = pa.RecordBatch.from_arrays([parent.column(0).slice(3, n), parent.column(1).slice(11, n), parent.column(2).slice(5, n)], names=["s", "t", "id"])
    check_forms(ctx, dev, host, FORMS[14:20] + FORMS[:3], "parts sliced differently")


# ---- more rows than one pass of the launch grids ------------------------------------------------------------------------------------
@pytest.mark.parametrize("nulls", [False, True], ids=["dense", "nulls"])
def test_more_rows_than_one_grid_pass(ctx, nulls):
    """2^21 + 65 rows of 0..3 bytes through the rows, scan and gather kernels.  (Expected values from pyarrow.compute, which the
    CPU tier pins to the reference on ASCII.)"""
    n = GRID_ROWS + 65
    rng = np.random.default_rng(5)
    lengths = rng.integers(0, 4, n)
    data = rng.choice(np.frombuffer(b"aB c", np.uint8), int(lengths.sum())).tobytes()
    offs = np.zeros(n + 1, np.int32)
    np.cumsum(lengths, out=offs[1:])
    valid = rng.random(n) < 0.9 if nulls else None
    bitmap = pa.py_buffer(np.packbits(valid, bitorder="little").tobytes()) if nulls else None
    s = pa.Array.from_buffers(pa.utf8(), n, [bitmap, pa.py_buffer(offs.tobytes()), pa.py_buffer(data)], null_count=int((~valid).sum()) if nulls else 0)
    host = pa.RecordBatch.from_arrays([s], names=["s"])
    dev = chq.DeviceRecordBatch.from_host(host, ctx)
    for sql, want in [("length(s)", pc.utf8_length(s)), ("octet_length(s)", pc.binary_length(s)), ("upper(s)", pc.ascii_upper(s)),
                      ("trim(s)", pc.utf8_trim(s, characters=" ")), ("substring(s from 2 for 1)", pc.utf8_slice_codeunits(s, 1, 2)),
                      ("s || '-' || s", pc.binary_join_element_wise(s, pa.scalar("-"), s, ""))]:
        got, _ = chq.compute_value(dev, [[]], parse_expr(sql), ctx=ctx)
        assert got.type == want.type and got.null_count == want.null_count and got.equals(want), sql
        if got.type == pa.utf8() and sql != "upper(s)":   # (the byte map keeps the bytes of null rows)
            total = int(np.frombuffer(got.buffers()[1], np.int32, n + 1)[-1])
            assert total == pc.sum(pc.binary_length(want)).as_py(), sql


def test_byte_map_more_bytes_than_one_grid_pass(ctx):
    rows, each = 1100, 16 * 1024
    rng = np.random.default_rng(8)
    data = rng.integers(32, 127, rows * each + 5, dtype=np.uint8).tobytes()
    assert len(data) > GRID_MAP_BYTES + 4096
    offs = (np.arange(rows + 1, dtype=np.int64) * each).astype(np.int32)
    offs[-1] += 5
    s = pa.Array.from_buffers(pa.utf8(), rows, [None, pa.py_buffer(offs.tobytes()), pa.py_buffer(data)], null_count=0)
    dev = chq.DeviceRecordBatch.from_host(pa.RecordBatch.from_arrays([s], names=["s"]), ctx)
    for sql, want in (("upper(s)", pc.ascii_upper(s)), ("lower(s)", pc.ascii_lower(s))):
        got, _ = chq.compute_value(dev.slice(1, rows - 1), [[]], parse_expr(sql), ctx=ctx)
        assert got.equals(want.slice(1)), sql


# ---- through the operators -------------------------------------------------------------------------------------------------------------
PREDICATES = [("upper(s) = 'AB'", lambda s, t: None if s is None else R.upper(s) == b"AB"),
              ("length(s) > 3", lambda s, t: None if s is None else R.length(s) > 3),
              ("s || 'x' like '%ax'", lambda s, t: None if s is None else (s + b"x").endswith(b"ax")),
              ("length(trim(s)) > 2 and id > 5", None)]


def operator_batches():
    return [batch(pool_cells(n, True, 30 + k) if n else [], seed=40 + k) for k, n in enumerate((257, 64, 1, 0, 130))]


def expected_rows(host, ref):
    """the rows a filter keeps: the Boolean column `m` computed by the reference, filtered by the CPU oracle"""
    s, t, ids = cells_of(host.column("s")), cells_of(host.column("t")), host.column("id").to_pylist()
    if ref is None:   # PREDICATES[3]
        mask = [None if a is None or i is None else (R.length(R.trim(a)) > 2 and i > 5) for a, i in zip(s, ids)]
    else:
        mask = [ref(a, b) for a, b in zip(s, t)]
    m = pa.array(mask, pa.bool_())
    plus = pa.RecordBatch.from_arrays(list(host.columns) + [m], schema=host.schema.append(pa.field("m", pa.bool_(), m.null_count > 0)))
    kept = O.filter_record(plus, empty_aliases(plus), parse_expr("m"))
    return pa.RecordBatch.from_arrays(kept.columns[:-1], schema=host.schema)


@pytest.mark.parametrize("sql,ref", PREDICATES, ids=[p[0] for p in PREDICATES])
def test_filter_record(ctx, sql, ref):
    for host in operator_batches():
        want = expected_rows(host, ref)
        al = empty_aliases(host)
        got = chq.filter_record(chq.DeviceRecordBatch.from_host(host, ctx), al, parse_expr(sql), ctx=ctx).to_host()
        assert batches_identical(got, want), f"{sql}, {host.num_rows} rows:\n{explain_diff(got, want)}"
        got = chq.filter_record(host, al, parse_expr(sql), ctx=ctx)
        assert batches_identical(got, want), f"{sql}, {host.num_rows} rows, host record:\n{explain_diff(got, want)}"


@pytest.mark.parametrize("sql,ref", PREDICATES[:3], ids=[p[0] for p in PREDICATES[:3]])
def test_filter_records(ctx, sql, ref):
    hosts = operator_batches()
    want = [expected_rows(h, ref) for h in hosts]
    al = empty_aliases(hosts[0])
    got = chq.filter_records([chq.DeviceRecordBatch.from_host(h, ctx) for h in hosts], al, parse_expr(sql), ctx=ctx)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert batches_identical(g.to_host(), w), f"{sql}, batch {i}:\n{explain_diff(g.to_host(), w)}"
    got = chq.filter_records(hosts, al, parse_expr(sql), ctx=ctx, device_result=False)
    for i, (g, w) in enumerate(zip(got, want)):
        assert batches_identical(g, w), f"{sql}, host batch {i}:\n{explain_diff(g, w)}"


@pytest.mark.parametrize("sql,ref", PREDICATES[:3], ids=[p[0] for p in PREDICATES[:3]])
def test_filter_project_record_gives_the_two_step_result(ctx, sql, ref):
    fields = parse_select("select id, s, upper(t) as u, length(s) as n from x").projection
    for host in operator_batches():
        al = empty_aliases(host)
        kept = expected_rows(host, ref)
        on_device = chq.filter_project_record(parse_expr(sql), fields, chq.DeviceRecordBatch.from_host(host, ctx), al, ctx=ctx).to_host()
        on_host = chq.filter_project_record(parse_expr(sql), fields, host, al, ctx=ctx, device_result=False)
        for got, what in ((on_device, "device batch"), (on_host, "host record")):
            what = f"{sql}, {host.num_rows} rows, {what}"
            assert got.schema.names == ["id", "s", "u", "n"] and got.num_rows == kept.num_rows, what
            assert [f.type for f in got.schema] == [pa.int32(), pa.utf8(), pa.utf8(), pa.int32()], what
            assert got.column(0).to_pylist() == kept.column("id").to_pylist() and cells_of(got.column(1)) == cells_of(kept.column("s")), what
            # (row by row: what the null slots of `u` enclose is whatever the filter left in those of `t`)
            assert cells_of(got.column(2)) == [None if b is None else R.upper(b) for b in cells_of(kept.column("t"))], f"{what}: u"
            if kept.num_rows:
                check_array(got.column(3), [None if a is None else R.length(a) for a in cells_of(kept.column("s"))], f"{what}: n")


def test_statuses_on_the_device(ctx):
    host = batch(pool_cells(10, True, 1))
    dev = chq.DeviceRecordBatch.from_host(host, ctx)
    al = empty_aliases(host)
    for sql, code in (("upper(id)", 22), ("s || id", 22), ("substring(s from id)", 30), ("substring(s from 1 for -1)", 22), ("upper(s, s)", 22)):
        with pytest.raises(chq.ChqError) as e:
            chq.compute_value(dev, al, parse_expr(sql), ctx=ctx)
        assert e.value.code == code, sql
    with pytest.raises(chq.ChqError) as e:      # a non-Boolean predicate answers as before, now that its value can be computed
        chq.filter_record(dev, al, parse_expr("length(s)"), ctx=ctx)
    assert e.value.code != 0
    with pytest.raises(chq.ChqError) as unknown:
        chq.compute_value(dev, al, parse_expr("foo(s)"), ctx=ctx)
    assert unknown.value.code == 2 and "Function(foo)" in str(unknown.value)


# ---- a Utf8 result past int32 offsets: refused before a byte is copied ---------------------------------------------------------------------
def test_utf8_byte_total_refusal(ctx):
    """forged offsets, no large allocation (tests/test_gpu_case.py has the same for CASE): two columns of two rows, each of which
    claims 2^30 bytes in one row.  strfn_rows_kernel reads offsets only for `||`, the total (2^31) is checked on the host, and
    the gather -- which would read the bytes -- never runs."""
    big = 2**30
    offs = pa.RecordBatch.from_arrays([pa.array([0, big, big], pa.int32()), pa.array([0, 0, big], pa.int32()), pa.array([1, 0, 0], pa.int32())], names=["so", "to", "c"])
    up = chq.DeviceRecordBatch.from_host(offs, ctx)
    data = up.column_buffer_address(2)      # 12 bytes that are never read
    dev = chq.DeviceRecordBatch.from_device_buffers([{"name": "s", "format": "u", "values": up.column_buffer_address(0), "data": data},
                                                     {"name": "t", "format": "u", "values": up.column_buffer_address(1), "data": data}], 2, ctx, keepalive=[up])
    with pytest.raises(chq.ChqError) as ei:
        chq.compute_value(dev, [[], []], parse_expr("s || t"), ctx=ctx)
    assert ei.value.code == 22 and "int32 offsets" in str(ei.value) and str(2**31) in str(ei.value)
