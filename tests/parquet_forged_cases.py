"""Named forged Parquet files for the page decoders of csrc/parquet.hip (tests/parquet_forge.py writes them).

Hybrid cases: build("<shape>/<v1|v2>-<none|snappy>").  A shape is a function that writes a run script into a Layout of a
given bit width and returns a check of where its runs ended up against the kernel's windows; the file holds a dictionary
Int32 column `i`, a dictionary Utf8 column `s` (forged index streams), an optional Int32 column `o` (forged definition
levels) and, with V2 pages, a Boolean column `b` (forged RLE values), each with the shape at its own bit width.
String cases: build("<shape>/<plain-v1-none|plain-v2-snappy|dict-snappy>"): PLAIN BYTE_ARRAY pages whose strings are chosen
with the position of the page in its chunk buffer, checked against the walk model."""
from __future__ import annotations

import numpy as np
import pyarrow as pa

from tests import parquet_forge as P
from tests.parquet_forge import HYB_USABLE as W, Forged, Layout

VARIANTS = ("v1-none", "v1-snappy", "v2-none", "v2-snappy")
DICT_BW = 11             # forged width of the dictionary columns unless the shape says otherwise (the dictionary needs 5)
DICT_SIZE = 23


class Report:
    """what became of a Layout: the stream, its runs as the strict decoder finds them, the windows of the kernel model"""

    def __init__(self, L: Layout, stream: bytes, n: int):
        self.L, self.stream, self.n, self.bw = L, stream, n, L.bw
        self.values, self.runs = P.decode(stream, L.bw, n)
        self.starts, self.parsed, self.emitted = P.restages(self.runs, len(stream), L.bw, n)
        assert self.emitted == n

    def at(self, mark: str, j: int = 0):
        i = self.L.marked(mark)[j]
        return self.runs[i], self.parsed[i]


# ---- shapes: fn(L) -> check(report) or None; L.tail: keywords of the closing Layout.finish -------------------------------------
def sh_widths(L):
    L.rle(300).bp(40, 2).rle(5).bp(3).rle(1)
    L.tail = dict(extra=13)


def sh_one_run(h, size):
    def fn(L):
        full = (W - h) // max(L.bw, 1)
        groups = {"short": 1000, "exact": full, "plus1": full + 1, "w5": 5 * W // max(L.bw, 1) + 3, "w50": 50 * W // max(L.bw, 1) + 3}[size]
        if size in ("exact", "plus1"):
            assert (W - h) % L.bw == 0, "the bit width must divide the window behind the header"
        L.tail = dict(n=groups * 8, header_width=h, mark="run")

        def check(r):
            assert len(r.runs) == 1 and r.runs[0].hdr == h and r.runs[0].count == groups
            want = {"short": 1, "exact": 1, "plus1": 2, "w5": 6, "w50": 51}[size]
            assert len(r.starts) == want, (len(r.starts), want)
            if size == "exact":
                assert h + groups * r.bw == W
            if size == "plus1":
                assert r.parsed[0].pieces == [(0, groups - 1), (1, 1)]
        return check
    return fn


def sh_bp_edge(d, ends):
    """a bit-packed run whose last whole group inside window 0 ends d bytes before the window end (d = -1: bw - 1); `ends`:
    the run ends there, else 100 more groups are pending"""
    def fn(L):
        dd = L.bw - 1 if d < 0 else d
        L.rle(10)
        start = 80 + (W - dd - 3 - 80) % L.bw
        L.fill_to(start)
        g = (W - dd - 3 - start) // L.bw
        L.bp(g + (0 if ends else 100), 3, mark="run")
        L.rle(9).bp(2)

        def check(r):
            run, p = r.at("run")
            assert p.window == 0 and p.wend == W and W - (run.pos + run.hdr + g * r.bw) == dd and p.pieces[0] == (0, g)
            assert len(p.pieces) == (1 if ends else 2)
            assert r.starts[1] == W - dd
        return check
    return fn


def sh_bp_starts_late(e):
    """a bit-packed run whose header lies e bytes before the end of window 0: parsed there only at e = 9, and then none of its
    groups fit (all pending)"""
    def fn(L):
        L.rle(10).bp_to(W - e)
        L.bp(50, 1, mark="run")
        L.rle(9)

        def check(r):
            run, p = r.at("run")
            assert W - run.pos == e
            if e >= P.HYB_EDGE and r.bw > e - 1:
                assert p.window == 0 and p.pieces == [(1, 50)] and r.starts[1] == run.pos + 1
            elif e < P.HYB_EDGE:
                assert p.window == 1 and p.wstart == run.pos
        return check
    return fn


def sh_rle_edge(d):
    """an RLE run (header padded to 5 bytes) whose header starts d bytes before the end of window 0"""
    def fn(L):
        L.rle(5).bp_to(W - d)
        L.rle(300, 5, mark="run")
        L.bp(4).rle(2)

        def check(r):
            run, p = r.at("run")
            assert W - run.pos == d and run.hdr == 5
            assert (p.window, p.wstart) == ((0, 0) if d >= P.HYB_EDGE else (1, run.pos))
        return check
    return fn


def sh_rle_count(c):
    def fn(L):
        L.bp(1).rle(c, mark="run").bp(2).rle(c if c < 1000 else 3)

        def check(r):
            assert r.at("run")[0].count == c and r.at("run")[0].hdr == len(P.varint(c << 1))
        return check
    return fn


def sh_bp_groups(g):
    def fn(L):
        L.rle(3).bp(g, mark="run").rle(2).bp(g)
        return lambda r: _assert(r.at("run")[0].count == g and not r.at("run")[0].rle)
    return fn


def sh_mix(seed):
    def fn(L):
        rng = np.random.default_rng(seed)
        long_bp = (W + 500) // max(L.bw, 1)
        for _ in range(70):
            hw = int(rng.integers(1, 6)) if rng.random() < 0.3 else None
            if rng.random() < 0.5:
                L.rle(int(rng.choice([1, 2, 5, 255, 256, 257, 1000, 5000])), max(hw or 0, 3) if hw else None)
            else:
                g = int(rng.choice([1, 2, 31, 32, 33, 100, 700, long_bp]))
                L.bp(g, max(hw, len(P.varint(g << 1 | 1))) if hw else None)
        L.tail = dict(extra=int(rng.integers(1, 60)))
        return lambda r: _assert(len(r.starts) >= 3, len(r.starts))
    return fn


def sh_alternating(L):
    for _ in range(4500):
        L.bp(1).rle(1)
    return lambda r: _assert(len(r.starts) >= 2 and len(r.runs) >= 9000, len(r.starts))


def sh_padded_varints(L):
    for hw in (2, 3, 4, 5):
        L.rle(7, hw).bp(3, hw)
    L.tail = dict(extra=5, header_width=5)
    return lambda r: _assert([x.hdr for x in r.runs] == [2, 2, 3, 3, 4, 4, 5, 5, 5])


def sh_rle_overshoot(L):
    L.bp(3).rle(20, declared=1000, mark="run")
    return lambda r: _assert(r.runs[-1].count == 1000 and r.n - r.runs[-1].first == 20)


def sh_junk_padding(L):
    L.rle(4)
    L.tail = dict(extra=8 * 30 + 3, junk=(1 << L.bw) - 1)

    def check(r):
        last = r.runs[-1]
        pad = P.unpack_bits(r.stream[last.pos + last.hdr:], r.bw, last.count * 8)[r.n - last.first:]
        assert len(pad) == 5 and (pad == (1 << r.bw) - 1).all() and (r.bw == 1 or pad[0] >= DICT_SIZE)
    return check


def sh_trailing_bytes(L):
    L.rle(4).bp(2)
    L.tail = dict(extra=19, trailing=b"\xff\x03\x80\x80\xff\xff\xff")
    return lambda r: _assert(r.runs[-1].pos + r.runs[-1].hdr + r.runs[-1].size == len(r.stream) - 7)


def sh_cut_off(long):
    """the last group of the page ends with the byte of the last real value (3 of its 8 values)"""
    def fn(L):
        L.rle(4)
        L.tail = dict(extra=8 * (2 * W // max(L.bw, 1) if long else 30) + 3, pad=False)

        def check(r):
            last = r.runs[-1]
            assert last.size == ((r.n - last.first) * r.bw + 7) // 8
            assert last.cut == (r.bw >= 2) and len(r.starts) == (3 if long else 1)
        return check
    return fn


def sh_all(value, rle):
    def fn(L):
        L.force = value
        if rle:
            L.rle(5000)
        else:
            L.tail = dict(n=5000, header_width=2)
        return lambda r: _assert(len(r.runs) == 1 and r.runs[0].rle == rle and (r.values == value).all())
    return fn


def sh_zero_rle(L):
    L.bp(2).rle(0, mark="run").rle(5).bp(1)


def sh_zero_bp(L):
    L.rle(6).bp(0, mark="run").rle(5).bp(1)


def sh_declared_beyond(L):
    L.rle(6)
    L.tail = dict(extra=8 * 12, declared_groups=12 + 5)


def _assert(ok, what=None):
    assert ok, what


def _shape(fn, cols="isob", bw=DICT_BW):
    return dict(fn=fn, cols=cols, bw=bw)


SHAPES = {}
for _bw in (0, 1, 2, 7, 8, 9, 15, 16, 17, 24, 25, 31, 32):
    SHAPES[f"bw{_bw}"] = _shape(sh_widths, "is", _bw)
for _h, _b in ((2, 14), (3, 15), (4, 4)):
    for _size in ("short", "exact", "plus1"):
        SHAPES[f"one_run_h{_h}_{_size}"] = _shape(sh_one_run(_h, _size), "is", _b)
        if _h > 2 or _size == "short":       # (at bit width 1 a window of groups needs a 3-byte header)
            SHAPES[f"one_run_h{_h}_{_size}_levels"] = _shape(sh_one_run(_h, _size), "ob")
SHAPES["one_run_h3_w5"] = _shape(sh_one_run(3, "w5"), "is", 24)
SHAPES["one_run_h4_w50"] = _shape(sh_one_run(4, "w50"), "is", 32)
SHAPES["one_run_h3_w5_levels"] = _shape(sh_one_run(3, "w5"), "ob")
for _d, _name in ((0, "0"), (1, "1"), (-1, "bw_less_1")):
    SHAPES[f"bp_group_ends_{_name}_before_window_end"] = _shape(sh_bp_edge(_d, False), "isob" if _d == 0 else "is")
SHAPES["bp_run_ends_at_window_end"] = _shape(sh_bp_edge(0, True))
for _e in (9, 8, 1):
    SHAPES[f"bp_starts_{_e}_before_window_end"] = _shape(sh_bp_starts_late(_e))
for _d in (9, 8, 5, 2, 1):
    for _vb, _b in ((1, 7), (2, 16), (3, 17), (4, 32)):
        SHAPES[f"rle_{_d}_before_window_end_vb{_vb}"] = _shape(sh_rle_edge(_d), "isob" if _vb == 1 else "is", _b)
for _c in (1, 255, 256, 257):
    SHAPES[f"rle_count_{_c}"] = _shape(sh_rle_count(_c))
SHAPES["rle_count_2m"] = _shape(sh_rle_count((1 << 21) + 3))
for _g in (1, 31, 32, 33):
    SHAPES[f"bp_groups_{_g}"] = _shape(sh_bp_groups(_g))
for _seed in range(4):
    SHAPES[f"mix_{_seed}"] = _shape(sh_mix(_seed))
SHAPES["alternating"] = _shape(sh_alternating)
SHAPES["padded_varints"] = _shape(sh_padded_varints)
SHAPES["rle_overshoot"] = _shape(sh_rle_overshoot)
SHAPES["junk_padding"] = _shape(sh_junk_padding)
SHAPES["trailing_bytes"] = _shape(sh_trailing_bytes)
SHAPES["cut_off_final_group"] = _shape(sh_cut_off(False))
SHAPES["cut_off_final_group_third_window"] = _shape(sh_cut_off(True), "is")
SHAPES["all_valid_rle"] = _shape(sh_all(1, True), "ob")
SHAPES["all_valid_bp"] = _shape(sh_all(1, False), "ob")
SHAPES["all_null"] = _shape(sh_all(0, True), "ob")

LENIENT_SHAPES = {"zero_count_rle": _shape(sh_zero_rle), "zero_group_bp": _shape(sh_zero_bp), "declared_groups_beyond_stream": _shape(sh_declared_beyond)}

CASES = [f"{s}/{v}" for s in SHAPES for v in VARIANTS]
LENIENT = [f"{s}/{v}" for s in LENIENT_SHAPES for v in ("v1-none", "v2-snappy")]
HOST_RESULT = [c for c in CASES if c.split("/")[0] in ("bw32", "one_run_h3_w5", "mix_1", "cut_off_final_group", "rle_9_before_window_end_vb4",
                                                       "bp_starts_9_before_window_end", "all_null", "junk_padding")]


# ---- files ------------------------------------------------------------------------------------------------------------------
def _writer(variant: str, cols) -> dict:
    ver, codec = variant.split("-")
    return dict(compression=codec, data_page_version={"v1": "1.0", "v2": "2.0"}[ver], use_dictionary=[c for c in cols if c in "is"],
                write_statistics=False, data_page_size=1 << 28, dictionary_pagesize_limit=1 << 22, row_group_size=1 << 26)


def _layouts(shape: dict, variant: str):
    cols = [c for c in shape["cols"] if c != "b" or variant.startswith("v2")]
    lays, checks = {}, {}
    for c in cols:
        L = Layout(shape["bw"] if c in "is" else 1)
        L.tail, L.force = {}, None
        checks[c] = shape["fn"](L)
        lays[c] = L
    n = max([L.tail["n"] if "n" in L.tail else L.k + L.tail.get("extra", 0) for L in lays.values()])
    for L in lays.values():
        kw = {k: v for k, v in L.tail.items() if k not in ("n", "extra")}
        if kw.get("declared_groups") is not None:
            kw["declared_groups"] += (n - L.k + 7) // 8 - 12
        L.finish(n, **kw)
    return lays, checks, n


def _table(lays: dict, n: int, seed: int):
    rng = np.random.default_rng(seed)
    arrays, fields, want = [], [], {}
    for c, L in lays.items():
        limit = min(1 << L.bw, DICT_SIZE)
        v = L.values(rng, limit) if L.force is None else np.full(n, L.force)
        want[c] = v
        if c == "i":
            a = pa.array((v * 1000003 + 7).astype(np.int32))
        elif c == "s":
            a = pa.array(np.array([f"str{j}" * (j % 3 + 1) for j in range(limit)], dtype=object)[v], type=pa.string())
        elif c == "o":
            a = pa.array(rng.integers(-2**31, 2**31, n).astype(np.int32), mask=v == 0)
        else:
            a = pa.array(v.astype(bool))
        arrays.append(a)
        fields.append(pa.field(c, a.type, nullable=c == "o"))
    return pa.table(arrays, schema=pa.schema(fields)), want


def _forge(lays: dict, n: int, variant: str, seed: int, damage=None, strict=True):
    """the table of the layouts written by pyarrow, every column's stream replaced by its layout's.  damage(col, stream) ->
    stream: what to store instead"""
    t, want = _table(lays, n, seed)
    names, streams = list(lays), {}

    def fn(sec: P.Section):
        c = names[sec.info.column]
        L = lays[c]
        if sec.version == 0:
            return None
        assert sec.info.page == (1 if c in "is" else 0) and sec.info.num_values == n, "one data page per column"
        if c in "is":
            old, head = sec.values[1:], b""
            idx = P.decode(old, sec.values[0], n)[0]     # (pyarrow numbers the dictionary by first appearance)
        elif c == "o":
            old, head = sec.levels, b""
            idx = P.decode(old, 1, n)[0]
            assert (idx == want[c]).all()
        else:
            ln = int.from_bytes(sec.values[:4], "little")
            assert ln == len(sec.values) - 4, "RLE boolean page"
            idx = P.decode(sec.values[4:], 1, n)[0]
            assert (idx == want[c]).all()
        s = L.stream(idx)
        if strict:
            assert (P.decode(s, L.bw, n)[0] == idx).all()
        streams[c] = (s, L.bw, n)
        if damage:
            s = damage(c, s)
        if c in "is":
            return None, (s if damage and getattr(damage, "whole", False) else bytes([L.bw]) + s)
        if c == "o":
            return s, None
        return None, (s if damage and getattr(damage, "whole", False) else len(s).to_bytes(4, "little") + s)
    raw = P.repack(P.write(t, **_writer(variant, names)), fn)
    assert set(streams) == set(names)
    return t, raw, streams


def build_hybrid(name: str) -> Forged:
    shape_name, variant = name.split("/")
    lenient = shape_name in LENIENT_SHAPES
    shape = (LENIENT_SHAPES if lenient else SHAPES)[shape_name]
    lays, checks, n = _layouts(shape, variant)
    t, raw, streams = _forge(lays, n, variant, seed=len(shape_name) * 7 + VARIANTS.index(variant), strict=not lenient)
    for c, L in lays.items():
        if lenient:
            try:
                P.decode(streams[c][0], L.bw, n)
            except P.HybridError:
                continue
            assert shape_name == "declared_groups_beyond_stream" and P.decode(streams[c][0], L.bw, n)[1][-1].cut
            continue
        r = Report(L, streams[c][0], n)
        if checks[c]:
            checks[c](r)
    return Forged(t, raw, streams, lenient=lenient)


# ---- damage -----------------------------------------------------------------------------------------------------------------
def _simple(cols, bw=DICT_BW):
    lays = {}
    for c in cols:
        L = Layout(bw if c in "is" else 1)
        L.force = None
        L.bp(20).rle(40).bp(6, 2)
        lays[c] = L
    return lays


def _damaged(cols, variant, last, damage, whole=False, bw=DICT_BW) -> Forged:
    """a three-run stream + `last(L)` in every column, stored after damage(col, stream)"""
    lays = _simple(cols, bw)
    for L in lays.values():
        last(L)
    n = max(L.k for L in lays.values())
    for L in lays.values():
        assert L.k == n
        L.finish(n)
    damage.whole = whole
    t, raw, streams = _forge(lays, n, variant, seed=11, damage=damage)
    return Forged(t, raw, streams, damaged=True)


def dm_ends_early():
    return _damaged("is", "v1-none", lambda L: L.bp(5), lambda c, s: s[:-5 * DICT_BW - 1])          # the last run is missing


def dm_cut_in_header():
    # (the byte that is left says "RLE, 50 repetitions" to a decoder that does not see that it asks for more header)
    return _damaged("is", "v2-none", lambda L: L.rle(50, 3), lambda c, s: s[:-2 - 2])


def dm_cut_in_rle_value():
    return _damaged("is", "v1-snappy", lambda L: L.rle(50), lambda c, s: s[:-1], bw=16)


def dm_bad_index(col, variant):
    def build():
        def damage(c, s):
            if c != col:
                return s
            at = 1 + 3 * DICT_BW          # the fourth group of the first run: its first value becomes DICT_SIZE
            g = P.unpack_bits(s[at:at + DICT_BW], DICT_BW, 8)
            g[0] = DICT_SIZE
            return s[:at] + P.pack_bits(g, DICT_BW) + s[at + DICT_BW:]
        return _damaged("is", variant, lambda L: L.bp(5), damage)
    return build


def dm_bit_width(bw):
    return lambda: _damaged("is", "v1-none", lambda L: L.bp(5), lambda c, s: bytes([bw]) + s, whole=True)


def dm_levels_short():
    return _damaged("o", "v1-none", lambda L: L.bp(5), lambda c, s: s[:-6])


def dm_levels_short_v2_snappy():
    return _damaged("o", "v2-snappy", lambda L: L.bp(5), lambda c, s: s[:-6])


def dm_bool_prefix():
    return _damaged("b", "v2-none", lambda L: L.bp(5), lambda c, s: (len(s) + 100).to_bytes(4, "little") + s, whole=True)


DAMAGED_BUILDERS = {
    "ends_before_n_values": dm_ends_early, "cut_inside_header": dm_cut_in_header, "cut_inside_rle_value": dm_cut_in_rle_value,
    "index_beyond_dictionary_int": dm_bad_index("i", "v1-none"), "index_beyond_dictionary_str": dm_bad_index("s", "v2-snappy"),
    "bit_width_33": dm_bit_width(33), "bit_width_255": dm_bit_width(255), "levels_shorter_than_rows": dm_levels_short,
    "levels_shorter_than_rows_v2_snappy": dm_levels_short_v2_snappy, "bool_length_prefix_past_page": dm_bool_prefix,
}


# ---- straight from pyarrow: many pages, pages without values -------------------------------------------------------------
def pg_empty_pages_between() -> Forged:
    """optional columns cut into pages of 256 rows; pages 3, 4 and 7 hold nulls only (value_base scan, n == 0 returns)"""
    rng = np.random.default_rng(5)
    n, per = 256 * 12, 256
    mask = rng.random(n) < 0.3
    for pg in (3, 4, 7):
        mask[pg * per:(pg + 1) * per] = True
    v = rng.integers(0, 20, n)
    t = pa.table({"i": pa.array(v.astype(np.int32), mask=mask), "s": pa.array(np.array([f"k{j}" for j in range(20)], dtype=object)[v], mask=mask, type=pa.string()),
                  "p": pa.array(rng.integers(0, 1 << 40, n), mask=mask), "b": pa.array(v % 2 == 0, mask=mask)})
    out = []
    for kw in (dict(compression="none"), dict(compression="snappy", data_page_version="2.0")):
        raw = P.write(t, use_dictionary=["i", "s"], data_page_size=1, write_batch_size=per, write_statistics=False, **kw)
        secs = [s for s in P.sections(raw) if s.version and s.info.column == 0]
        nonnull = [int(P.decode(s.levels, 1, s.info.num_values)[0].sum()) for s in secs]
        assert len(secs) == 12 and [k for k, c in enumerate(nonnull) if c == 0] == [3, 4, 7], nonnull
        out.append(raw)
    return out


def pg_many_pages() -> list:
    """more than 256 data pages in a chunk (pq_page_scan_kernel carries across its blocks of 256 pages)"""
    rng = np.random.default_rng(6)
    per, n_pages = 24, 700
    n = per * n_pages
    mask = rng.random(n) < 0.4
    v = rng.integers(0, 9, n)
    t = pa.table({"i": pa.array(v.astype(np.int32), mask=mask), "s": pa.array(np.array([f"w{j}" * j for j in range(9)], dtype=object)[v], mask=mask, type=pa.string()),
                  "p": pa.array(rng.integers(0, 1 << 40, n), mask=mask)})
    out = []
    for kw in (dict(compression="none", data_page_version="2.0"), dict(compression="snappy")):
        raw = P.write(t, use_dictionary=["i", "s"], data_page_size=1, write_batch_size=per, write_statistics=False, **kw)
        for c in range(3):
            assert len([s for s in P.sections(raw) if s.version and s.info.column == c]) == n_pages
        out.append(raw)
    return out


PYARROW_FILES = {"empty_pages_between": pg_empty_pages_between, "more_than_256_pages": pg_many_pages}


# ---- PLAIN BYTE_ARRAY pages ---------------------------------------------------------------------------------------------------
BA_VARIANTS = ("plain-v1-none", "plain-v2-snappy", "dict-snappy")


def _text(rng, ln: int, tag: int) -> bytes:
    """ln bytes of ASCII that no other value of the page shares (the tag leads where it fits)"""
    head = b"%07x" % tag
    body = bytes(rng.integers(0x61, 0x7b, max(ln - len(head), 0)).astype(np.uint8))
    return (head + body)[:ln] if ln >= len(head) else (head[-ln:] if ln else b"")


def _ba_file(strings, variant: str):
    t = pa.table({"s": pa.array([s.decode() for s in strings], type=pa.string())}, schema=pa.schema([pa.field("s", pa.string(), nullable=False)]))
    kind, _, rest = variant.partition("-")
    if kind == "dict":
        assert len(set(strings)) == len(strings), "a dictionary page holds every string once"
        raw = P.write(t, compression="snappy", use_dictionary=True, data_page_size=1 << 28, dictionary_pagesize_limit=1 << 26, write_statistics=False)
        page = 0
    else:
        ver, codec = rest.split("-")
        raw = P.write(t, compression=codec, use_dictionary=False, data_page_size=1 << 28, data_page_version={"v1": "1.0", "v2": "2.0"}[ver], write_statistics=False)
        page = 0
    img, at = P.chunk_image(raw, 0)
    pa_ = at[page]
    assert pa_.section.version == (0 if kind == "dict" else int(rest[1])) and pa_.section.values == b"".join(len(s).to_bytes(4, "little") + s for s in strings)
    assert img[pa_.values_at:pa_.values_at + pa_.values_len] == pa_.section.values
    return t, raw, img, pa_


def build_ba(name: str) -> Forged:
    shape, variant = name.split("/")
    fn = BA_SHAPES[shape]
    dict_page = variant.startswith("dict")
    a = 64
    for _ in range(4):        # (the position of the values follows from the header's length, which follows from the sizes)
        strings, check = fn(a, dict_page)
        t, raw, img, at = _ba_file(strings, variant)
        if at.values_at == a:
            break
        a = at.values_at
    else:
        raise AssertionError("the page's position does not settle")
    w = P.walk(img, at.values_at, at.values_len, len(strings))
    true = at.values_at + np.cumsum([0] + [4 + len(s) for s in strings[:-1]])
    assert not w.failed and w.values == len(strings) and np.array_equal(w.positions, true), "the walk model loses the page"
    check(w, at, true)
    return Forged(t, raw, {"s": (at.section.values, 0, len(strings))})


def _wlim(a: int) -> int:
    return (a & ~15) + P.WALK_WINDOW


def ba_prefix_at(e):
    """ragged strings; a length prefix starts e bytes before the end of window 0 (e = 1, 2, 3: it straddles; 0: the value in
    front ends exactly there; 4: the prefix ends exactly there)"""
    def fn(a, dict_page):
        rng = np.random.default_rng(40 + e)
        lens = [int(x) for x in rng.integers(7 if dict_page else 0, 40, 3000)]
        pos = a + np.cumsum([0] + [4 + x for x in lens])
        target = _wlim(a) - e
        j = int(np.searchsorted(pos, target - 60))       # value j - 1 is stretched so that value j's prefix starts at the target
        lens[j - 1] += target - int(pos[j])
        strings = [_text(rng, x, i) for i, x in enumerate(lens)]

        def check(w, at, true):
            assert target in true and len(w.windows) >= 2
            assert w.windows[0] == (a & ~15, P.WALK_WINDOW)
            assert w.windows[1][0] == (target & ~15 if e < 4 else w.windows[1][0])
            if e == 4:
                assert w.windows[1][0] > target
        return strings, check
    return fn


def ba_uniform(ln, n):
    def fn(a, dict_page):
        rng = np.random.default_rng(ln)
        lead = 8 + (1 - a) % 4       # (one value in front: the uniform ones then start off the window's 4-byte grid)
        strings = [_text(rng, lead, n)] + [_text(rng, ln, i) for i in range(n)]

        def check(w, at, true):
            assert len(w.windows) >= 3 and all(s.length == ln for s in w.steps[1:])
            cut = [s for s in w.steps[1:] if s.total < P.WALK_STEP and s.k + s.total < n + 1]
            assert cut and all(s.q + s.total * (4 + ln) + 4 > sum(w.windows[s.window]) for s in cut), "steps cut by the window end"
        return strings, check
    return fn


def ba_broken(lane):
    """uniform strings of 8 bytes; value 768 + lane, the one lane `lane` of the fourth step guesses, has 9"""
    def fn(a, dict_page):
        rng = np.random.default_rng(lane)
        strings = [_text(rng, 9 if i == 768 + lane else 8, i) for i in range(2000)]

        def check(w, at, true):
            s = [x for x in w.steps if x.k == 768]
            assert len(s) == 1 and s[0].window == 0
            assert (s[0].length, s[0].total) == ((9, 1) if lane == 0 else (8, lane))
        return strings, check
    return fn


def ba_imitation(real):
    """value 0 .. real - 1 have 8 bytes; value `real` has 300, and its bytes spell a length prefix of 8 wherever a lane guesses
    one; behind it uniform values again.  The first step confirms `real` values and none of the imitations"""
    def fn(a, dict_page):
        rng = np.random.default_rng(real)
        strings = [_text(rng, 8, i) for i in range(real)]
        big = bytearray(_text(rng, 300, 9999))
        at0 = a + real * 12 + 4                  # where the long value's bytes start
        for lane in range(real + 1, real + 26):
            off = a + lane * 12 - at0
            if 0 <= off and off + 4 <= len(big):
                big[off:off + 4] = (8).to_bytes(4, "little")
        strings.append(bytes(big))
        strings += [_text(rng, 8, 20000 + i) for i in range(600)]

        def check(w, at, true):
            img_guess = [a + lane * 12 for lane in range(real + 1, real + 20)]
            assert all(g not in true for g in img_guess)
            assert at.section.values[img_guess[3] - a:img_guess[3] - a + 4] == (8).to_bytes(4, "little")
            assert w.steps[0].k == 0 and w.steps[0].total == real and w.steps[1].length == (300 if real > 1 else 8)
        return strings, check
    return fn


def ba_ragged_bursts(a, dict_page):
    rng = np.random.default_rng(77)
    lens = []
    for ragged, uniform in ((100, 600), (30, 300), (49, 256), (200, 0)):
        lens += [int(x) for x in rng.integers(8, 30, ragged)] + [12] * uniform
    strings = [_text(rng, x, i) for i, x in enumerate(lens)]

    def check(w, at, true):
        full = [i for i, s in enumerate(w.steps) if s.burst == P.WALK_BURST]
        assert full and any(w.steps[i + 1].total > 1 for i in full if i + 1 < len(w.steps)), "a burst that is left for a confirmed step"
        assert any(s.total == P.WALK_STEP for s in w.steps)
        assert true[-1] + 4 + len(strings[-1]) == at.values_at + at.values_len and w.steps[-1].burst > 0, "the last value ends the page, inside a burst"
    return strings, check


BA_SHAPES = {f"prefix_{e}_before_window_end": ba_prefix_at(e) for e in (1, 2, 3, 0, 4)}
BA_SHAPES["uniform_13_across_windows"] = ba_uniform(13, 9000)
BA_SHAPES["uniform_empty"] = ba_uniform(0, 20000)
for _lane in (0, 1, 63, 64, 255):
    BA_SHAPES[f"uniform_broken_at_lane_{_lane}"] = ba_broken(_lane)
BA_SHAPES["imitated_prefixes_behind_value_1"] = ba_imitation(1)
BA_SHAPES["imitated_prefixes_behind_value_5"] = ba_imitation(5)
BA_SHAPES["ragged_bursts_to_page_end"] = ba_ragged_bursts
BA_CASES = [f"{s}/{v}" for s in BA_SHAPES for v in BA_VARIANTS if not (s == "uniform_empty" and v.startswith("dict"))]


def _ba_damaged(how: str, variant: str) -> Forged:
    rng = np.random.default_rng(9)
    strings = [_text(rng, int(x), i) for i, x in enumerate(rng.integers(8, 30, 500))]
    t, raw, _, _ = _ba_file(strings, variant)

    def fn(sec: P.Section):
        if (sec.version == 0) != variant.startswith("dict"):
            return None
        v = bytearray(sec.values)
        if how == "prefix_past_end":
            at = sum(4 + len(s) for s in strings[:400])
            v[at:at + 4] = (len(v) - at - 3).to_bytes(4, "little")
        elif how == "one_byte_short":
            v = v[:-1]
        else:
            v = v[:len(v) - 4 - len(strings[-1])]
        return None, bytes(v)
    return Forged(t, P.repack(raw, fn), {}, damaged=True)


for _how, _v in (("prefix_past_end", "plain-v1-none"), ("one_byte_short", "plain-v2-snappy"), ("fewer_values_than_n", "plain-v1-none"),
                 ("one_byte_short", "dict-snappy"), ("prefix_past_end", "dict-snappy")):
    DAMAGED_BUILDERS[f"strings_{_how}/{_v}"] = (lambda h, v: lambda: _ba_damaged(h, v))(_how, _v)

DAMAGED = list(DAMAGED_BUILDERS)


def good_file() -> Forged:
    return build("mix_0/v2-snappy")


def build(name: str) -> Forged:
    if name in DAMAGED_BUILDERS:
        return DAMAGED_BUILDERS[name]()
    if name.split("/")[0] in BA_SHAPES:
        return build_ba(name)
    return build_hybrid(name)
