"""Forged RLE / bit-packed hybrid streams and PLAIN BYTE_ARRAY pages at chosen positions (pure Python + numpy, no GPU).

Arrow's hybrid encoder only writes bit-packed runs of at most 63 groups (a one-byte header), minimal varints and the bit
width the dictionary needs.  The format allows, and other writers produce, bit-packed runs of any length, padded varints,
bit width 0 and widths up to 32; the serial decoders of csrc/parquet.hip (hybrid_decode_block, pq_ba_walk_kernel) have
window-edge rules that only such streams reach.  This module writes any run script, decodes streams strictly, models where
the kernels restage their LDS windows, and puts forged level / values sections into the pages of a file pyarrow wrote.

  Rle / BitPacked, encode / decode   run scripts <-> hybrid streams (any header width, declared groups, cut-off last group)
  restages                           where hybrid_decode_block starts its windows and at which window end each run is parsed
  repack                             a file whose data pages get new level / values sections (V1 / V2, uncompressed / snappy)
  chunk_image / values_at / walk     the chunk buffer the decode kernels see, a page's values in it, pq_ba_walk_kernel's steps
  Layout                             a run script planned by stream position before the data exists
The Thrift reader / writer and the page walker are those of tests/snappy_forge.py."""
from __future__ import annotations

import re
from dataclasses import dataclass, field
from typing import Callable, List, Optional, Tuple

import numpy as np
import pyarrow as pa

from tests.snappy_forge import (DATA_PAGE, DATA_PAGE_V2, DICTIONARY_PAGE, SNAPPY, PageInfo, TReader, footer, pa_decompress, pages,
                                rewrite, varint, write)

# ---- the kernels' numbers (csrc/parquet.hip), checked against the source by tests/test_parquet_forge.py ------------------
HYB_WINDOW = 16384       # PQ_HYB_WINDOW
HYB_SPARE = 16           # bytes of the window never filled
HYB_USABLE = HYB_WINDOW - HYB_SPARE
HYB_EDGE = 9             # a run header nearer than this to the window end is parsed after a restage
HYB_BLOCK = 256          # PQ_HYB_BLOCK: values per pass of the workgroup
WALK_WINDOW = 32768      # PQ_WALK_WINDOW
WALK_SPEC = 4            # PQ_WALK_SPEC: guessed positions per lane and step
WALK_STEP = 64 * WALK_SPEC
WALK_BURST = 48          # serial steps after a speculative step that confirmed one value

SOURCE_PATTERNS = {      # name -> regular expression whose group 1 is the value in parquet.hip
    "HYB_WINDOW": r"constexpr int PQ_HYB_WINDOW = (\d+);",
    "HYB_SPARE": r"\(uint32_t\)\(PQ_HYB_WINDOW - (\d+)\) \? len - pos",
    "HYB_EDGE": r"if \(pos \+ (\d+) > wend && wend < len\) break;",
    "HYB_BLOCK": r"constexpr int PQ_HYB_BLOCK = (\d+);",
    "WALK_WINDOW": r"constexpr int PQ_WALK_WINDOW = (\d+);",
    "WALK_SPEC": r"constexpr int PQ_WALK_SPEC = (\d+);",
    "WALK_BURST": r"for \(int burst = 0; burst < (\d+) && k < n; \+\+burst\)",
}


def source_constants(text: str) -> dict:
    out = {}
    for name, pat in SOURCE_PATTERNS.items():
        m = re.findall(pat, text)
        assert len(m) == 1, f"{name}: {len(m)} matches of {pat!r} in parquet.hip"
        out[name] = int(m[0])
    return out


# ---- run scripts ------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Rle:
    """`count` repetitions of `value`; header_width pads the header varint to so many bytes"""
    count: int
    value: int
    header_width: Optional[int] = None


@dataclass(frozen=True, eq=False)
class BitPacked:
    """values in groups of 8.  declared_groups: what the header says (default: the groups the values fill); pad=True fills
    the last group with zeros, pad=False ends the run with the last value's byte (a cut-off final group)"""
    values: object
    header_width: Optional[int] = None
    declared_groups: Optional[int] = None
    pad: bool = True


class HybridError(ValueError):
    pass


def vbytes(bw: int) -> int:
    return (bw + 7) // 8


def pack_bits(values, bw: int) -> bytes:
    """values, bw bits each, LSB first; the last byte padded with zero bits"""
    v = np.asarray(values, dtype=np.uint64)
    if bw == 0 or len(v) == 0:
        return b""
    bits = ((v[:, None] >> np.arange(bw, dtype=np.uint64)) & np.uint64(1)).astype(np.uint8)
    return np.packbits(bits.reshape(-1), bitorder="little").tobytes()


def unpack_bits(data: bytes, bw: int, count: int) -> np.ndarray:
    if bw == 0:
        return np.zeros(count, dtype=np.uint64)
    bits = np.unpackbits(np.frombuffer(data, dtype=np.uint8), bitorder="little")[:count * bw].reshape(count, bw)
    return (bits.astype(np.uint64) << np.arange(bw, dtype=np.uint64)).sum(axis=1, dtype=np.uint64)


def encode_run(r, bw: int) -> bytes:
    if isinstance(r, Rle):
        assert 0 <= r.value < max(1 << bw, 1) or bw == 0 and r.value == 0
        return varint(r.count << 1, r.header_width) + int(r.value).to_bytes(vbytes(bw), "little")
    v = np.asarray(r.values, dtype=np.uint64)
    groups = (len(v) + 7) // 8
    declared = groups if r.declared_groups is None else r.declared_groups
    if r.pad:
        v = np.concatenate([v, np.zeros(groups * 8 - len(v), dtype=np.uint64)])
    return varint(declared << 1 | 1, r.header_width) + pack_bits(v, bw)


def encode(runs, bw: int) -> bytes:
    return b"".join(encode_run(r, bw) for r in runs)


@dataclass
class RunAt:
    """a run as the strict decoder met it"""
    pos: int             # of its header
    hdr: int             # header bytes
    rle: bool
    count: int           # RLE: declared repetitions; bit-packed: declared groups
    size: int            # bytes behind the header that belong to it (a cut-off last group: fewer than count * bw)
    first: int           # index of its first value
    cut: bool = False


def decode(stream: bytes, bw: int, n: int) -> Tuple[np.ndarray, List[RunAt]]:
    """strict: the first n values and every run read to get them.  Raises HybridError on a header cut off or wider than 5
    bytes, an RLE value cut off, a run of zero repetitions or groups, a bit width above 32, and a stream that ends before n
    values.  A bit-packed run may end with the stream inside its last group if the bytes hold the values still wanted (cut);
    an RLE run may count past n; bytes behind the last value are not looked at"""
    if not 0 <= bw <= 32:
        raise HybridError(f"bit width {bw}")
    stream = bytes(stream)
    out = np.zeros(n, dtype=np.uint64)
    runs: List[RunAt] = []
    pos = k = 0
    while k < n:
        at, h, sh = pos, 0, 0
        while True:
            if pos >= len(stream):
                raise HybridError(f"stream ends inside the header at {at} ({k} of {n} values)")
            if pos - at >= 5:
                raise HybridError(f"header at {at} wider than 5 bytes")
            b = stream[pos]
            pos += 1
            h |= (b & 0x7F) << sh
            sh += 7
            if not b & 0x80:
                break
        if h >> 1 == 0:
            raise HybridError(f"run of zero {'groups' if h & 1 else 'repetitions'} at {at}")
        if h & 1 == 0:
            if pos + vbytes(bw) > len(stream):
                raise HybridError(f"stream ends inside the RLE value at {pos}")
            v = int.from_bytes(stream[pos:pos + vbytes(bw)], "little")
            if v >> bw:
                raise HybridError(f"RLE value {v} at {pos} wider than {bw} bits")
            runs.append(RunAt(at, pos - at, True, h >> 1, vbytes(bw), k))
            pos += vbytes(bw)
            cnt = min(h >> 1, n - k)
            out[k:k + cnt] = v
            k += cnt
            continue
        groups = h >> 1
        want = min(groups * 8, n - k)
        size = groups * bw
        cut = False
        if pos + size > len(stream):
            size = len(stream) - pos
            cut = True
            if bw and size * 8 // bw < want:
                raise HybridError(f"bit-packed run at {at} declares {groups} groups, the stream holds {size * 8 // bw} values of them")
        runs.append(RunAt(at, pos - at, False, groups, size, k, cut))
        out[k:k + want] = unpack_bits(stream[pos:pos + (want * bw + 7) // 8], bw, want)
        k += want
        pos += size
    return out, runs


# ---- where hybrid_decode_block restages -------------------------------------------------------------------------------------
@dataclass
class Parsed:
    """a run's header as the kernel parses it: in window `window` (that starts at `wstart` and ends at `wend`)"""
    window: int
    wstart: int
    wend: int
    pieces: list = field(default_factory=list)   # bit-packed: (window, groups expanded there)


def restages(runs: List[RunAt], length: int, bw: int, n: int):
    """the control flow of hybrid_decode_block over the runs of a well-formed stream of `length` bytes: (window starts,
    [Parsed per run], values emitted).  Window 0 starts at byte 0, every later one where the inner loop broke"""
    starts, parsed = [], []
    pos = k = pending = i = 0
    vb = vbytes(bw)
    while k < n and pos < length:
        starts.append(pos)
        wend = pos + min(length - pos, HYB_USABLE)
        stop = False
        while k < n and pos < wend and not stop:
            if pending:
                groups, pending = pending, 0
            else:
                if pos + HYB_EDGE > wend and wend < length:
                    break
                r = runs[i]
                assert r.pos == pos, (r.pos, pos)
                parsed.append(Parsed(len(starts) - 1, starts[-1], wend))
                i += 1
                pos += r.hdr
                if r.rle:
                    pos += vb
                    k += min(r.count, n - k)
                    continue
                groups = r.count
            fit = (wend - pos) // bw if bw else groups
            now = min(groups, fit)
            if now < groups and wend >= length:      # the stream ends inside this run: the values its last bytes hold
                k += min((wend - pos) * 8 // bw, n - k)
                parsed[i - 1].pieces.append((len(starts) - 1, now))
                stop = True
                break
            if now == 0:
                pending = groups
                break
            parsed[i - 1].pieces.append((len(starts) - 1, now))
            k += min(now * 8, n - k)
            pos += now * bw
            if now < groups:
                pending = groups - now
                break
        if stop:
            break
    return starts, parsed, k


# ---- a file whose data pages get new sections -------------------------------------------------------------------------------
@dataclass
class Section:
    """a page handed to repack's callback, inflated and taken apart"""
    info: PageInfo
    version: int                 # 0 dictionary page, 1 / 2 data page
    optional: bool
    levels: Optional[bytes]      # definition levels without the V1 length prefix (None: required column / dictionary page)
    values: bytes


def _deflate(b: bytes) -> bytes:
    return pa.Codec("snappy").compress(b, asbytes=True)


def _optional(meta, ci: int) -> bool:
    schema = meta.get(2)[1]
    assert len(schema) == 1 + schema[0].get(5), "flat schemas only"
    return schema[1 + ci].get(3) == 1


def _take_apart(meta, info: PageInfo, payload: bytes) -> Section:
    ph, snappy = info.header, info.codec == SNAPPY
    assert info.codec in (0, SNAPPY)
    opt = _optional(meta, info.column)
    if info.type == DATA_PAGE_V2:
        h2 = ph.get(8)
        info.num_values = h2.get(1)
        dl = h2.get(5, 0)
        assert h2.get(6, 0) == 0
        vals = payload[dl:]
        if snappy and h2.get(7, True):
            vals = pa_decompress(vals, ph.get(2) - dl)
        return Section(info, 2, opt, payload[:dl] if opt else None, vals)
    data = pa_decompress(payload, ph.get(2)) if snappy else payload
    if info.type == DICTIONARY_PAGE:
        info.num_values = ph.get(7).get(1)
        return Section(info, 0, opt, None, data)
    assert info.type == DATA_PAGE
    info.num_values = ph.get(5).get(1)
    if not opt:
        return Section(info, 1, opt, None, data)
    l = int.from_bytes(data[:4], "little")
    return Section(info, 1, opt, data[4:4 + l], data[4 + l:])


def repack(raw: bytes, fn: Callable[[Section], Optional[tuple]]) -> bytes:
    """`raw` (written by pyarrow uncompressed or with snappy, flat schema) with the sections of every page replaced by
    fn(section) = (levels or None, values or None); None keeps the page.  Everything that follows from the new lengths is
    rewritten: the V1 level length prefix, definition_levels_byte_length of V2 headers, both page sizes, and through
    snappy_forge.rewrite the chunk sizes, page offsets and row-group sizes of the footer"""
    meta = footer(raw)

    def page_fn(info: PageInfo, payload: bytes):
        sec = _take_apart(meta, info, payload)
        got = fn(sec)
        if got is None:
            return None
        lv = sec.levels if got[0] is None else got[0]
        vs = sec.values if got[1] is None else got[1]
        ph, snappy = info.header, info.codec == SNAPPY
        if sec.version == 2:
            h2 = ph.get(8)
            lv = lv or b""
            h2.set(5, len(lv))
            ph.set(2, len(lv) + len(vs))
            return lv + (_deflate(vs) if snappy and h2.get(7, True) else vs)
        data = (len(lv).to_bytes(4, "little") + lv if sec.optional and sec.version == 1 else b"") + vs
        ph.set(2, len(data))
        return _deflate(data) if snappy else data
    return rewrite(raw, page_fn, None)


def sections(raw: bytes) -> List[Section]:
    meta = footer(raw)
    out = []
    for info, payload in pages(raw):
        info.codec = meta.get(4)[1][info.row_group].get(1)[1][info.column].get(3).get(4)
        out.append(_take_apart(meta, info, payload))
    return out


# ---- the chunk buffer the decode kernels see (parquet_scan.cpp) ---------------------------------------------------------------
@dataclass
class PageAt:
    section: Section
    values_at: int       # of the values section (dictionary page: dict_at) in the chunk buffer / the image
    values_len: int


def chunk_image(raw: bytes, column: int = 0, row_group: int = 0) -> Tuple[bytes, List[PageAt]]:
    """the bytes `p.chunk` points at for one column chunk and where each page's values lie in them.  Uncompressed: the
    chunk as it lies in the file (positions relative to its first page header).  Snappy: the image the inflate kernels
    write -- every page at the next multiple of 16, a V2 page's values section in a slot of its own behind its levels"""
    meta = footer(raw)
    md = meta.get(4)[1][row_group].get(1)[1][column].get(3)
    snappy = md.get(4) == SNAPPY
    start = md.get(11) if md.get(11) else md.get(9)
    img = bytearray(raw[start:start + md.get(7)]) if not snappy else bytearray()
    out, pos, image_at = [], start, 0
    for info, payload in pages(raw):
        if (info.row_group, info.column) != (row_group, column):
            continue
        info.codec = md.get(4)
        sec = _take_apart(meta, info, payload)
        usize = info.header.get(2)
        r = TReader(raw, pos)
        r.struct()
        rel = r.p - start
        pos = r.p + info.header.get(3)
        lv = len(sec.levels or b"")
        if not snappy:
            at = rel + (4 + lv if sec.version == 1 and sec.optional else lv if sec.version == 2 else 0)
            out.append(PageAt(sec, at, len(sec.values)))
            continue
        rel = image_at
        image_at += (usize + 15) // 16 * 16
        if sec.version == 2:
            vrel = image_at
            image_at += (usize - lv + 15) // 16 * 16
            img += bytes(image_at - len(img))
            img[rel:rel + lv] = sec.levels or b""
            img[vrel:vrel + len(sec.values)] = sec.values
            out.append(PageAt(sec, vrel, len(sec.values)))
        else:
            img += bytes(image_at - len(img))
            data = (lv.to_bytes(4, "little") + sec.levels if sec.version == 1 and sec.optional else b"") + sec.values
            img[rel:rel + len(data)] = data
            out.append(PageAt(sec, rel + len(data) - len(sec.values), len(sec.values)))
    return bytes(img), out


def values_at(raw: bytes, column: int = 0, row_group: int = 0, page: int = 0) -> PageAt:
    return chunk_image(raw, column, row_group)[1][page]


# ---- pq_ba_walk_kernel's steps ----------------------------------------------------------------------------------------------
@dataclass
class Step:
    q: int               # position of the length prefix the step starts at
    k: int               # values found before it
    length: int          # L
    total: int           # values the speculation confirmed
    window: int
    burst: int = 0       # serial steps that followed (total == 1)


@dataclass
class Walk:
    windows: list        # (wbase, wbytes)
    steps: List[Step]
    values: int
    failed: bool
    positions: np.ndarray    # of the length prefixes found


def walk(chunk: bytes, at: int, length: int, n: int) -> Walk:
    """the control flow of pq_ba_walk_kernel on a page of n values at chunk[at : at + length]"""
    buf = np.frombuffer(bytes(chunk) + bytes(64), dtype=np.uint8).astype(np.uint64)

    def length_at(p):
        p = np.asarray(p, dtype=np.int64)
        return buf[p] | buf[p + 1] << np.uint64(8) | buf[p + 2] << np.uint64(16) | buf[p + 3] << np.uint64(24)
    end, q, k, failed = at + length, at, 0, False
    windows, steps, found = [], [], []
    lane = np.arange(64, dtype=np.int64)
    while k < n and not failed:
        wbase = q & ~15
        wlim = wbase + min(end - wbase, WALK_WINDOW)
        windows.append((wbase, wlim - wbase))
        while k < n:
            if q + 4 > end:
                failed = True
                break
            if q + 4 > wlim:
                break
            L = int(length_at(q))
            if L > end - q - 4:
                failed = True
                break
            total = 0
            for j in range(WALK_SPEC):
                c = q + (j * 64 + lane) * (4 + L)
                ok = (k + j * 64 + lane < n) & (c + 4 <= wlim) & (c + 4 + L <= end)
                ok[ok] = length_at(c[ok]) == L
                cnt = 64 if ok.all() else int(np.argmin(ok))
                found.extend(int(x) for x in c[:cnt])
                total += cnt
                if cnt < 64:
                    break
            steps.append(Step(q, k, L, total, len(windows) - 1))
            k += total
            q += total * (4 + L)
            if total == 1:
                for _ in range(WALK_BURST):
                    if k >= n:
                        break
                    if q + 4 > end:
                        failed = True
                        break
                    if q + 4 > wlim:
                        break
                    L2 = int(length_at(q))
                    if L2 > end - q - 4:
                        failed = True
                        break
                    found.append(q)
                    steps[-1].burst += 1
                    k += 1
                    q += 4 + L2
                if failed:
                    break
    return Walk(windows, steps, k, failed, np.asarray(found, dtype=np.int64))


# ---- run scripts planned by stream position -------------------------------------------------------------------------------
@dataclass
class Seg:
    rle: bool
    values: int                      # values of the page it stands for (an RLE run that overshoots: fewer than `count`)
    count: int                       # RLE: declared repetitions; bit-packed: groups the values fill
    header_width: Optional[int] = None
    declared_groups: Optional[int] = None
    pad: bool = True
    junk: Optional[int] = None       # bit-packed: value of the padding behind the last real value
    mark: Optional[str] = None


class Layout:
    """a run script written front to back BEFORE the values exist: `pos` counts the stream's bytes, `k` its values.  RLE runs
    ask for a constant stretch of values (`const`); bit-packed runs take whatever values lie there"""

    def __init__(self, bw: int):
        self.bw, self.vb = bw, vbytes(bw)
        self.segs: List[Seg] = []
        self.pos = self.k = 0
        self.const: List[Tuple[int, int]] = []
        self.trailing = b""
        self.closed = False

    def _hdr(self, h: int, width: Optional[int]) -> int:
        return len(varint(h, width))

    def rle(self, count: int, header_width: Optional[int] = None, declared: Optional[int] = None, mark: Optional[str] = None):
        """`count` values as one RLE run (declared: the repetitions its header states, >= count)"""
        declared = count if declared is None else declared
        assert declared >= count >= 0
        self.segs.append(Seg(True, count, declared, header_width, mark=mark))
        self.const.append((self.k, count))
        self.pos += self._hdr(declared << 1, header_width) + self.vb
        self.k += count
        return self

    def bp(self, groups: int, header_width: Optional[int] = None, mark: Optional[str] = None):
        """`groups` whole groups as one bit-packed run"""
        self.segs.append(Seg(False, groups * 8, groups, header_width, mark=mark))
        self.pos += self._hdr(groups << 1 | 1, header_width) + groups * self.bw
        self.k += groups * 8
        return self

    def fill_to(self, at: int):
        """runs (one long bit-packed one, then count-1 RLE runs of chosen header widths) up to stream byte `at` exactly"""
        assert at >= self.pos
        lo, hi = 1 + self.vb, 5 + self.vb
        reserve = lo * hi + 8
        if self.bw and at - self.pos > reserve + 5 + self.bw:
            self.bp((at - self.pos - reserve - 5) // self.bw)
        left = at - self.pos
        while left:
            runs_left = -(-left // hi)
            assert runs_left * lo <= left, (left, lo, hi)
            size = min(hi, left - (runs_left - 1) * lo)
            self.rle(1, size - self.vb)
            left -= size
        assert self.pos == at
        return self

    def bp_to(self, at: int, header_width: int = 3):
        """filler, then one bit-packed run of many groups that ends at stream byte `at` exactly (so that what follows is
        the first thing the kernel meets there)"""
        base = self.pos + 80
        start = base + (at - header_width - base) % self.bw
        self.fill_to(start)
        self.bp((at - header_width - start) // self.bw, header_width)
        assert self.pos == at
        return self

    def finish(self, n: int, header_width: Optional[int] = None, pad: bool = True, junk: Optional[int] = None,
               declared_groups: Optional[int] = None, trailing: bytes = b"", mark: Optional[str] = None):
        """the values still missing up to n as one last bit-packed run (none if k == n already)"""
        assert not self.closed and n >= self.k
        if n > self.k:
            v = n - self.k
            self.segs.append(Seg(False, v, (v + 7) // 8, header_width, declared_groups, pad, junk, mark))
            self.k = n
        self.trailing = trailing
        self.closed = True
        return self

    def values(self, rng: np.random.Generator, limit: int) -> np.ndarray:
        """random values below `limit` with the constant stretches the RLE runs need"""
        v = rng.integers(0, max(limit, 1), self.k)
        for k, c in self.const:
            v[k:k + c] = v[k] if c else 0
        return v

    def runs(self, values) -> list:
        values = np.asarray(values)
        assert self.closed and len(values) == self.k
        out, k = [], 0
        for s in self.segs:
            part = values[k:k + s.values]
            k += s.values
            if s.rle:
                v = int(part[0]) if s.values else 0
                assert (part == v).all(), "an RLE run over values that differ"
                out.append(Rle(s.count, v, s.header_width))
            else:
                if s.junk is not None:
                    part = np.concatenate([part, np.full(-len(part) % 8, s.junk, dtype=part.dtype)])
                out.append(BitPacked(part, s.header_width, s.declared_groups, s.pad))
        return out

    def stream(self, values) -> bytes:
        return encode(self.runs(values), self.bw) + self.trailing

    def marked(self, mark: str) -> List[int]:
        return [i for i, s in enumerate(self.segs) if s.mark == mark]


@dataclass
class Forged:
    """a file with forged sections, the table it must read as, and what the builders asserted about each forged stream"""
    table: pa.Table
    raw: bytes
    streams: dict = field(default_factory=dict)    # column name -> (stream, bit width, values wanted)
    damaged: bool = False
    lenient: bool = False
    note: str = ""


__all__ = ["write", "Forged", "Layout", "Rle", "BitPacked"]
