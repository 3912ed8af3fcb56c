"""Forged snappy streams and Parquet files that carry them (pure Python + numpy, no GPU).

Google's compressor (what `pa.Codec("snappy")` and every Parquet writer we test with use) only emits canonical streams:
64 KiB blocks, copies of length >= 4 through the copy-1 / copy-2 tags, offsets below 64 KiB, minimal literal headers and no
element across a block boundary.  The format (format_description.txt of google/snappy) allows much more, and the inflate
kernels of csrc/parquet_codec.hip have branches for all of it.  This module writes any legal (or deliberately damaged)
element script, decodes streams strictly, and puts forged streams into the pages of a file pyarrow wrote, so that the GPU
tests can compare the scan with pyarrow's reader on the same bytes.

  encode / decode     element scripts <-> raw snappy streams (every tag, every literal header width, padded preambles)
  canonical / respell the elements of the compressor's stream, and re-spellings of them that produce the same bytes
  repack              a snappy Parquet file whose pages are re-compressed by a callback (Thrift compact protocol in Python)
  Plan                the scan planner's numbers (parquet_scan_plan.cpp): which path a page takes, its segment bounds
"""
from __future__ import annotations

import io
from dataclasses import dataclass, field
from typing import Callable, List, Optional

import numpy as np
import pyarrow as pa


# ---- elements ------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Lit:
    """a literal; `nb`: bytes of extended length behind the tag (0: the length sits in the tag, 1..4: tags 60..63);
    None = the minimal header"""
    data: bytes
    nb: Optional[int] = None

    @property
    def length(self) -> int:
        return len(self.data)


@dataclass(frozen=True)
class Copy:
    """a copy of `length` bytes from `offset` bytes back; `kind`: 1 / 2 / 4 bytes of offset (tags 01, 10, 11); None = the
    shortest tag that can hold it"""
    length: int
    offset: int
    kind: Optional[int] = None


@dataclass(frozen=True)
class Element:
    """an element as a decoder met it: where its header starts in the input, where its output starts"""
    kind: int            # 0 literal, 1 / 2 / 4 copy with so many offset bytes
    in_pos: int
    hdr: int             # header bytes (literal data follows them)
    out_pos: int
    length: int
    offset: int = 0
    nb: int = 0          # literal: extended-length bytes


class SnappyError(ValueError):
    pass


def min_nb(length: int) -> int:
    n = length - 1
    return 0 if n < 60 else 1 if n < 1 << 8 else 2 if n < 1 << 16 else 3 if n < 1 << 24 else 4


def min_kind(length: int, offset: int) -> int:
    if 4 <= length <= 11 and offset < 2048:
        return 1
    return 2 if offset < 65536 else 4


def varint(v: int, width: Optional[int] = None) -> bytes:
    """little-endian base-128; `width` pads it with continuation bytes (at most 5, what a 32-bit length may take)"""
    out = bytearray()
    while True:
        out.append(v & 0x7F)
        v >>= 7
        if v == 0:
            break
    if width is not None:
        if not len(out) <= width <= 5:
            raise ValueError(f"preamble of {len(out)} bytes cannot be {width} wide")
        out += bytes(width - len(out))
    for i in range(len(out) - 1):
        out[i] |= 0x80
    return bytes(out)


def encode_element(e) -> bytes:
    if isinstance(e, Lit):
        n = len(e.data) - 1
        nb = min_nb(len(e.data)) if e.nb is None else e.nb
        if n < 0 or nb < min_nb(len(e.data)) or nb > 4:
            raise ValueError(f"literal of {len(e.data)} bytes with {nb} length bytes")
        head = bytes([n << 2]) if nb == 0 else bytes([(59 + nb) << 2]) + n.to_bytes(nb, "little")
        return head + e.data
    kind = min_kind(e.length, e.offset) if e.kind is None else e.kind
    if kind == 1:
        if not (4 <= e.length <= 11 and 0 <= e.offset < 2048):
            raise ValueError(f"copy-1 of length {e.length}, offset {e.offset}")
        return bytes([1 | (e.length - 4) << 2 | (e.offset >> 8) << 5, e.offset & 0xFF])
    if not 1 <= e.length <= 64:
        raise ValueError(f"copy of length {e.length}")
    if kind == 2:
        if not 0 <= e.offset < 1 << 16:
            raise ValueError(f"copy-2 of offset {e.offset}")
        return bytes([2 | (e.length - 1) << 2]) + e.offset.to_bytes(2, "little")
    if kind == 4:
        return bytes([3 | (e.length - 1) << 2]) + e.offset.to_bytes(4, "little")
    raise ValueError(f"copy kind {kind}")


def out_len(elems) -> int:
    return sum(e.length for e in elems)


def encode(elems, dlen: Optional[int] = None, preamble: Optional[int] = None) -> bytes:
    """the raw stream of an element script; `dlen` overrides the declared length (damage), `preamble` pads its varint"""
    head = varint(out_len(elems) if dlen is None else dlen, preamble)
    return head + b"".join(encode_element(e) for e in elems)


def decode(src: bytes, expect: Optional[int] = None):
    """strict reference decoder: (output, [Element]).  Raises SnappyError on a truncated preamble or header, a literal past
    the input, offset 0, an offset beyond the output so far, output past the declared length, bytes after the last element,
    or (with `expect`) a declared length other than `expect`"""
    src = bytes(src)
    n = len(src)
    pos = dlen = sh = 0
    while True:
        if pos >= n or pos >= 5:
            raise SnappyError("truncated preamble")
        b = src[pos]
        pos += 1
        dlen |= (b & 0x7F) << sh
        sh += 7
        if not b & 0x80:
            break
    if dlen >= 1 << 32:
        raise SnappyError("declared length beyond 32 bits")
    if expect is not None and dlen != expect:
        raise SnappyError(f"declared length {dlen}, expected {expect}")
    out = bytearray()
    elems: List[Element] = []
    while pos < n:
        at, tag = pos, src[pos]
        kind = tag & 3
        if kind == 0:
            t6 = tag >> 2
            nb = t6 - 59 if t6 >= 60 else 0
            if pos + 1 + nb > n:
                raise SnappyError(f"truncated literal header at {pos}")
            ln = (int.from_bytes(src[pos + 1:pos + 1 + nb], "little") if nb else t6) + 1
            hdr = 1 + nb
            if pos + hdr + ln > n:
                raise SnappyError(f"literal at {pos} runs past the input")
            if len(out) + ln > dlen:
                raise SnappyError(f"literal at {pos} runs past the declared length")
            elems.append(Element(0, at, hdr, len(out), ln, 0, nb))
            out += src[pos + hdr:pos + hdr + ln]
            pos += hdr + ln
            continue
        hdr = {1: 2, 2: 3, 3: 5}[kind]
        if pos + hdr > n:
            raise SnappyError(f"truncated copy header at {pos}")
        if kind == 1:
            ln, off = ((tag >> 2) & 7) + 4, (tag >> 5) << 8 | src[pos + 1]
        else:
            ln, off = (tag >> 2) + 1, int.from_bytes(src[pos + 1:pos + hdr], "little")
        if off == 0:
            raise SnappyError(f"copy at {pos} with offset 0")
        if off > len(out):
            raise SnappyError(f"copy at {pos} reaches {off} back from output byte {len(out)}")
        if len(out) + ln > dlen:
            raise SnappyError(f"copy at {pos} runs past the declared length")
        elems.append(Element({1: 1, 2: 2, 3: 4}[kind], at, hdr, len(out), ln, off))
        start = len(out) - off
        if off >= ln:
            out += out[start:start + ln]
        else:                        # (a copy that reads what it writes: byte by byte)
            for i in range(ln):
                out.append(out[start + i])
        pos += hdr
    if len(out) != dlen:
        raise SnappyError(f"stream ends after {len(out)} of {dlen} bytes")
    return bytes(out), elems


def script(elems: List[Element], src: bytes) -> list:
    """decoded elements back to an element script that spells them the same way"""
    out = []
    for e in elems:
        if e.kind == 0:
            out.append(Lit(src[e.in_pos + e.hdr:e.in_pos + e.hdr + e.length], e.nb))
        else:
            out.append(Copy(e.length, e.offset, e.kind))
    return out


def pa_decompress(stream: bytes, dlen: int) -> bytes:
    return pa.Codec("snappy").decompress(stream, decompressed_size=dlen, asbytes=True)


def canonical(data: bytes) -> list:
    """the element script Google's compressor writes for `data`"""
    stream = pa.Codec("snappy").compress(data, asbytes=True)
    out, elems = decode(stream)
    assert out == data
    return script(elems, stream)


def positions(elems, pre: Optional[int] = None) -> List[Element]:
    """where every element of a script lies in its stream (no damage allowed) -- decode(encode(elems, preamble=pre))[1]"""
    return decode(encode(elems, preamble=pre))[1]


# ---- re-spellings: the same output, other elements -------------------------------------------------------------------------
def split_copy(c: Copy, lengths) -> list:
    """a copy cut into consecutive copies of the given lengths (same offset: each piece reads what the whole one would)"""
    assert sum(lengths) == c.length
    return [Copy(k, c.offset, c.kind if c.kind != 1 or 4 <= k <= 11 else None) for k in lengths]


def respell(elems, rng: np.random.Generator, copy4=0.3, short=0.2, wide=0.3, split_lit=0.2) -> list:
    """a random re-spelling: copies through copy-4 tags, copies cut into pieces of length 1 to 3, literals with wider
    headers than they need, literals cut in two"""
    out = []
    for e in elems:
        if isinstance(e, Copy):
            pieces = [e]
            if rng.random() < short and e.length >= 2:
                lens, left = [], e.length
                while left > 0:
                    k = min(left, int(rng.integers(1, 4)))
                    lens.append(k)
                    left -= k
                pieces = split_copy(Copy(e.length, e.offset), lens)
            for p in pieces:
                if rng.random() < copy4:
                    p = Copy(p.length, p.offset, 4)
                elif p.kind == 1 and rng.random() < copy4:
                    p = Copy(p.length, p.offset, 2)
                out.append(p)
        else:
            parts = [e.data]
            if rng.random() < split_lit and len(e.data) >= 2:
                k = int(rng.integers(1, len(e.data)))
                parts = [e.data[:k], e.data[k:]]
            for d in parts:
                nb = min_nb(len(d))
                if rng.random() < wide:
                    nb = int(rng.integers(max(nb, 1), 5))
                out.append(Lit(d, nb))
    return out


def grow(elems, k: int, lo: int = 0, hi: Optional[int] = None) -> list:
    """the same output in exactly `k` more input bytes, taken from elements [lo, hi): literal headers widened (+1 a step)
    and copies moved to wider tags (copy-1 -> copy-2 +1, copy-2 -> copy-4 +2)"""
    out = list(elems)
    hi = len(out) if hi is None else hi
    i = lo
    while k > 0:
        if i >= hi:
            raise ValueError(f"{k} more bytes cannot be taken from elements [{lo}, {hi})")
        e = out[i]
        if isinstance(e, Lit):
            nb = min_nb(len(e.data)) if e.nb is None else e.nb
            step = min(4 - nb, k)
            out[i] = Lit(e.data, nb + step)
            k -= step
        else:
            kind = min_kind(e.length, e.offset) if e.kind is None else e.kind
            if kind == 1:
                out[i], k = Copy(e.length, e.offset, 2), k - 1
                continue           # (the same element can grow again)
            if kind == 2 and k >= 2:
                out[i], k = Copy(e.length, e.offset, 4), k - 2
        i += 1
    return out


# ---- the scan planner's numbers (parquet_scan_plan.cpp, parquet_codec.hip) ----------------------------------------------------
SEGMENTS = 16            # PQ_SNAPPY_SEGMENTS
LEAD = 2048              # PQ_SNAPPY_LEAD
BLOCK = 65536            # output bytes per BLOCK job and of the LDS ring
LARGE = 512 << 10        # compressed bytes from which a page joins the wave's "large" chain
RING_NEAR = BLOCK - 64   # offsets up to this are read from the LDS ring, larger ones from HBM (wave_copy)


@dataclass
class Plan:
    """how the scan inflates a snappy page of `slen` compressed and `dlen` uncompressed bytes under option snappy_blocks"""
    slen: int
    dlen: int
    snappy_blocks: int = 1

    @property
    def indexed(self) -> bool:       # INDEX (or SEG + RESOLVE) + one BLOCK job per 64 KiB + FINISH
        return self.snappy_blocks != 0 and self.dlen >= 3 * BLOCK

    @property
    def large(self) -> bool:
        return self.indexed and self.slen >= LARGE

    @property
    def n_seg(self) -> int:          # >= 2: the walk runs in segments
        return min(SEGMENTS, self.slen >> 15) if self.indexed and self.snappy_blocks != 3 else 1

    def bound(self, w: int) -> int:  # b_w: where segment w's range of input starts
        return self.slen * w // self.n_seg

    def bounds(self) -> List[int]:
        return [self.bound(w) for w in range(1, self.n_seg)] if self.n_seg >= 2 else []


def element_at(elems: List[Element], in_pos: int) -> Element:
    """the element whose header or literal bytes hold input byte `in_pos`"""
    lo, hi = 0, len(elems)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if elems[mid].in_pos <= in_pos:
            lo = mid
        else:
            hi = mid
    return elems[lo]


def block_crossers(elems: List[Element]) -> List[Element]:
    return [e for e in elems if e.out_pos // BLOCK != (e.out_pos + e.length - 1) // BLOCK]


def below_block(elems: List[Element]) -> List[Element]:
    """copies whose source starts in an earlier 64 KiB block of output than the copy itself"""
    return [e for e in elems if e.kind and (e.out_pos - e.offset) // BLOCK < e.out_pos // BLOCK]


# ---- Thrift compact protocol: a generic reader / writer (field ids kept, unknown fields copied) --------------------------
T_TRUE, T_FALSE, T_BYTE, T_I16, T_I32, T_I64, T_DOUBLE, T_BINARY, T_LIST, T_SET, T_MAP, T_STRUCT = range(1, 13)


@dataclass
class TStruct:
    fields: list = field(default_factory=list)     # [fid, type, value]; a struct value is a TStruct, a list (etype, [values])

    def get(self, fid, default=None):
        for f in self.fields:
            if f[0] == fid:
                return f[2] if f[1] not in (T_TRUE, T_FALSE) else f[1] == T_TRUE
        return default

    def has(self, fid) -> bool:
        return any(f[0] == fid for f in self.fields)

    def set(self, fid, value, ty=None):
        for f in self.fields:
            if f[0] == fid:
                if f[1] in (T_TRUE, T_FALSE):
                    f[1] = T_TRUE if value else T_FALSE
                else:
                    f[2] = value
                return
        if ty is None:
            raise KeyError(fid)
        if ty in (T_TRUE, T_FALSE):
            ty, value = (T_TRUE if value else T_FALSE), None
        self.fields.append([fid, ty, value])
        self.fields.sort(key=lambda f: f[0])


class TReader:
    def __init__(self, buf: bytes, pos: int = 0):
        self.b, self.p = buf, pos

    def byte(self) -> int:
        v = self.b[self.p]
        self.p += 1
        return v

    def uvarint(self) -> int:
        v = sh = 0
        while True:
            c = self.byte()
            v |= (c & 0x7F) << sh
            sh += 7
            if not c & 0x80:
                return v

    def zigzag(self) -> int:
        v = self.uvarint()
        return (v >> 1) ^ -(v & 1)

    def value(self, ty):
        if ty in (T_TRUE, T_FALSE):
            return None
        if ty == T_BYTE:
            return self.byte()
        if ty in (T_I16, T_I32, T_I64):
            return self.zigzag()
        if ty == T_DOUBLE:
            v = self.b[self.p:self.p + 8]
            self.p += 8
            return v
        if ty == T_BINARY:
            n = self.uvarint()
            v = self.b[self.p:self.p + n]
            self.p += n
            return v
        if ty in (T_LIST, T_SET):
            h = self.byte()
            n, et = h >> 4, h & 15
            if n == 15:
                n = self.uvarint()
            # (booleans inside a list are one byte each)
            return (et, [self.byte() if et in (T_TRUE, T_FALSE) else self.value(et) for _ in range(n)])
        if ty == T_MAP:
            n = self.uvarint()
            if n == 0:
                return (0, 0, [])
            h = self.byte()
            kt, vt = h >> 4, h & 15
            return (kt, vt, [(self.value(kt), self.value(vt)) for _ in range(n)])
        if ty == T_STRUCT:
            return self.struct()
        raise ValueError(f"thrift type {ty}")

    def struct(self) -> TStruct:
        s, last = TStruct(), 0
        while True:
            h = self.byte()
            if h == 0:
                return s
            ty, delta = h & 15, h >> 4
            fid = last + delta if delta else self.zigzag()
            s.fields.append([fid, ty, self.value(ty)])
            last = fid


class TWriter:
    def __init__(self):
        self.o = bytearray()

    def uvarint(self, v: int):
        while True:
            if v < 0x80:
                self.o.append(v)
                return
            self.o.append(v & 0x7F | 0x80)
            v >>= 7

    def zigzag(self, v: int):
        self.uvarint((v << 1) ^ (v >> 63))

    def value(self, ty, v):
        if ty in (T_TRUE, T_FALSE):
            return
        if ty == T_BYTE:
            self.o.append(v)
        elif ty in (T_I16, T_I32, T_I64):
            self.zigzag(v)
        elif ty == T_DOUBLE:
            self.o += v
        elif ty == T_BINARY:
            self.uvarint(len(v))
            self.o += v
        elif ty in (T_LIST, T_SET):
            et, items = v
            if len(items) < 15:
                self.o.append(len(items) << 4 | et)
            else:
                self.o.append(0xF0 | et)
                self.uvarint(len(items))
            for x in items:
                if et in (T_TRUE, T_FALSE):
                    self.o.append(x)
                else:
                    self.value(et, x)
        elif ty == T_MAP:
            kt, vt, items = v
            self.uvarint(len(items))
            if items:
                self.o.append(kt << 4 | vt)
                for k, x in items:
                    self.value(kt, k)
                    self.value(vt, x)
        elif ty == T_STRUCT:
            self.struct(v)
        else:
            raise ValueError(f"thrift type {ty}")

    def struct(self, s: TStruct):
        last = 0
        for fid, ty, v in s.fields:
            if 0 < fid - last <= 15:
                self.o.append((fid - last) << 4 | ty)
            else:
                self.o.append(ty)
                self.zigzag(fid)
            self.value(ty, v)
            last = fid
        self.o.append(0)


def thrift_bytes(s: TStruct) -> bytes:
    w = TWriter()
    w.struct(s)
    return bytes(w.o)


# ---- Parquet: pages re-compressed in place ---------------------------------------------------------------------------------
DATA_PAGE, DICTIONARY_PAGE, DATA_PAGE_V2 = 0, 2, 3
SNAPPY = 1


@dataclass
class PageInfo:
    row_group: int
    column: int
    page: int              # index inside its chunk
    type: int              # DATA_PAGE / DICTIONARY_PAGE / DATA_PAGE_V2
    num_values: int
    uncompressed: int      # bytes of the section handed to the callback (V2: the values section only)
    levels: bytes = b""    # V2: the stored level sections in front of it
    header: TStruct = None
    codec: int = 1         # of its chunk (0 uncompressed, 1 snappy)


@dataclass
class Stored:
    """callback result for a V2 page: store the values section uncompressed (is_compressed = false)"""
    data: bytes


def footer(raw: bytes) -> TStruct:
    n = int.from_bytes(raw[-8:-4], "little")
    return TReader(raw, len(raw) - 8 - n).struct()


def rewrite(raw: bytes, page_fn: Callable[[PageInfo, bytes], Optional[bytes]], codec: Optional[int] = SNAPPY) -> bytes:
    """the page walker behind repack (and tests/parquet_forge.py): `raw` (written by pyarrow, no page index) with every
    page's stored payload replaced by page_fn(info, payload) -- None keeps it.  page_fn may change info.header (sizes of the
    sections, flags); compressed_page_size is set here, and the footer gets the chunks' moved offsets and new sizes.
    `codec`: the compression every chunk must have (None: any; info.codec says which)"""
    assert raw[:4] == b"PAR1" and raw[-4:] == b"PAR1"
    meta = footer(raw)
    out = bytearray(b"PAR1")
    for gi, rg in enumerate(meta.get(4)[1]):
        cols = rg.get(1)[1]
        rg_start, rg_size, rg_usize = None, 0, 0
        for ci, cc in enumerate(cols):
            md = cc.get(3)
            assert codec is None or md.get(4) == codec, "repack wants a snappy chunk"
            for fid in (10, 14):        # index page, bloom filter: not written by the tests' writer settings
                assert not md.has(fid)
            for fid in (4, 5, 6, 7):    # offset / column index
                assert not cc.has(fid), "repack wants a file without a page index"
            start = md.get(11) if md.get(11) else md.get(9)
            size = md.get(7)
            new_start = len(out)
            moved = {start: new_start}
            pos, page, dsize = start, 0, 0
            while pos < start + size:
                r = TReader(raw, pos)
                ph = r.struct()
                hdr_end = r.p
                csize, usize, ptype = ph.get(3), ph.get(2), ph.get(1)
                payload = raw[hdr_end:hdr_end + csize]
                assert not ph.has(4), "page CRCs are not rewritten"
                info = PageInfo(gi, ci, page, ptype, 0, usize, b"", ph, md.get(4))
                body = page_fn(info, payload)
                if body is None:
                    body = payload
                ph.set(3, len(body))
                head = thrift_bytes(ph)
                moved[pos] = len(out)
                dsize += len(head) - (hdr_end - pos) + ph.get(2) - usize
                out += head + body
                pos = hdr_end + csize
                page += 1
            assert pos == start + size, "pages do not tile their chunk"
            new_size = len(out) - new_start
            moved[start + size] = len(out)
            md.set(7, new_size)
            md.set(6, md.get(6) + dsize)
            md.set(9, moved[md.get(9)])
            if md.get(11):
                md.set(11, moved[md.get(11)])
            if cc.has(2):
                cc.set(2, moved[cc.get(2)] if cc.get(2) in moved else cc.get(2))
            rg_start = new_start if rg_start is None else rg_start
            rg_size += new_size
            rg_usize += dsize
        if rg.has(5):
            rg.set(5, rg_start)
        if rg.has(6):
            rg.set(6, rg_size)
        rg.set(2, rg.get(2) + rg_usize)  # total_byte_size: the chunks' uncompressed sizes
    foot = thrift_bytes(meta)
    out += foot + len(foot).to_bytes(4, "little") + b"PAR1"
    return bytes(out)


def repack(raw: bytes, fn: Callable[[PageInfo, bytes], object]) -> bytes:
    """`raw` (written by pyarrow with compression="snappy", no page index) with every page's snappy payload replaced by
    fn(info, inflated bytes): a new raw stream (bytes), Stored(data) for a V2 values section kept uncompressed, or None to
    keep the page as it is.  Page headers get their new compressed_page_size; the footer its moved offsets and sizes"""
    def page_fn(info: PageInfo, payload: bytes):
        ph, usize = info.header, info.uncompressed
        if info.type == DATA_PAGE_V2:
            h2 = ph.get(8)
            info.num_values = h2.get(1)
            lv = h2.get(5, 0) + h2.get(6, 0)
            info.levels, values = payload[:lv], payload[lv:]
            info.uncompressed = usize - lv
            if h2.get(7, True):
                values = pa_decompress(values, usize - lv)
            got = fn(info, values)
            if isinstance(got, Stored):
                h2.set(7, False, T_FALSE)
                return info.levels + got.data
            if got is not None:
                if h2.has(7):      # (pyarrow stores a values section that does not shrink: compressed now)
                    h2.set(7, True)
                return info.levels + got
            return None
        sub = ph.get(5) if info.type == DATA_PAGE else ph.get(7)
        info.num_values = sub.get(1)
        got = fn(info, pa_decompress(payload, usize))
        assert not isinstance(got, Stored), "only V2 pages store their values section uncompressed"
        return got
    return rewrite(raw, page_fn, SNAPPY)


def pages(raw: bytes):
    """(PageInfo, compressed payload) of every page of a file, in file order"""
    meta = footer(raw)
    for gi, rg in enumerate(meta.get(4)[1]):
        for ci, cc in enumerate(rg.get(1)[1]):
            md = cc.get(3)
            start = md.get(11) if md.get(11) else md.get(9)
            pos, page = start, 0
            while pos < start + md.get(7):
                r = TReader(raw, pos)
                ph = r.struct()
                payload = raw[r.p:r.p + ph.get(3)]
                yield PageInfo(gi, ci, page, ph.get(1), 0, ph.get(2), b"", ph), payload
                pos = r.p + ph.get(3)
                page += 1


def write(t: pa.Table, **kw) -> bytes:
    import pyarrow.parquet as pq
    kw.setdefault("compression", "snappy")
    kw.setdefault("max_rows_per_page", 1 << 24)     # (pages are cut by data_page_size alone)
    buf = io.BytesIO()
    pq.write_table(t, buf, **kw)
    return buf.getvalue()


# ---- stream builders: element scripts with chosen shapes at chosen input / output positions -------------------------------
class Builder:
    """an element script written front to back.  `size` counts the stream's bytes so far, the preamble included (written
    `pre` bytes wide, so that input positions are known before the output length is); `out` the bytes of output"""

    def __init__(self, rng: np.random.Generator, pre: int = 4, max_off: int = 60000, copy4: float = 0.15, short: float = 0.1):
        self.rng, self.pre, self.max_off, self.copy4, self.short = rng, pre, max_off, copy4, short
        self.elems: list = []
        self.size, self.out = pre, 0
        self.marks: dict = {}            # name -> indices of the elements a test is about

    def add(self, e, mark: Optional[str] = None):
        if mark:
            self.marks.setdefault(mark, []).append(len(self.elems))
        self.elems.append(e)
        self.size += len(encode_element(e))
        self.out += e.length
        return self

    def lit(self, data: bytes, nb: Optional[int] = None, mark: Optional[str] = None):
        return self.add(Lit(bytes(data), nb), mark)

    def copy(self, length: int, offset: int, kind: Optional[int] = None, mark: Optional[str] = None):
        assert 0 < offset <= self.out
        return self.add(Copy(length, offset, kind), mark)

    def one(self):
        """one random element: a short literal or a copy from up to max_off back (some through copy-4, some of length 1-3)"""
        r = self.rng
        if self.out < 16 or r.random() < 0.35:
            return self.lit(r.bytes(int(r.integers(1, 25))))
        off = int(r.integers(1, min(self.out, self.max_off) + 1))
        ln = int(r.integers(1, 4)) if r.random() < self.short else int(r.integers(4, 65))
        return self.copy(ln, off, 4 if r.random() < self.copy4 else None)

    def to_out(self, at: int):
        """random elements up to output byte `at` exactly (the last one a literal)"""
        while self.out < at - 80:
            self.one()
        if at > self.out:
            self.lit(self.rng.bytes(at - self.out))
        assert self.out == at
        return self

    def to_in(self, at: int):
        """random elements up to input byte `at` exactly (the next element starts there)"""
        lo = len(self.elems)
        while self.size < at - 80:
            self.one()
        assert self.size <= at and len(self.elems) - lo >= 8, (self.size, at)
        k = at - self.size
        self.elems[lo:] = grow(self.elems[lo:], k)
        self.size += k
        assert self.size == at
        return self

    def end(self, slen: Optional[int] = None) -> bytes:
        """the stream: output padded to whole 8-byte values (an Int64 column's PLAIN page), `slen` bytes long if asked"""
        if slen is not None:
            self.to_in(slen - 20)
        pad = -self.out % 8 or 8
        self.lit(self.rng.bytes(pad))
        if slen is not None:
            self.elems[-12:] = grow(self.elems[-12:], slen - self.size)
            self.size = slen
        s = encode(self.elems, preamble=self.pre)
        assert len(s) == self.size and (slen is None or len(s) == slen)
        return s

    def element(self, mark: str, k: int = 0) -> Element:
        """where a marked element ended up (call after end())"""
        return self.positions()[self.marks[mark][k]]

    def positions(self) -> List[Element]:
        return positions(self.elems, self.pre)


@dataclass
class Forged:
    """a file whose snappy pages were forged, and the table pyarrow wrote into it"""
    table: pa.Table
    raw: bytes
    streams: list = field(default_factory=list)    # (PageInfo, forged stream) of every page the callback replaced
    damaged: bool = False


def int64_table(data: bytes) -> pa.Table:
    """a required Int64 column whose PLAIN values are `data`: its V1 / V2 data page is exactly these bytes"""
    v = pa.array(np.frombuffer(data, dtype=np.int64))
    return pa.table({"v": v}, schema=pa.schema([pa.field("v", pa.int64(), nullable=False)]))


def forge_int64(stream: bytes, damaged_from: Optional[bytes] = None, **kw) -> Forged:
    """the page of a one-page Int64 column replaced by `stream`.  damaged_from: the valid stream whose output the table
    holds (`stream` is then damage the scan must report)"""
    data = decode(damaged_from if damaged_from is not None else stream)[0]
    t = int64_table(data)
    kw.setdefault("use_dictionary", False)
    kw.setdefault("data_page_size", 1 << 26)
    got = []

    def fn(info, b):
        assert info.type != DICTIONARY_PAGE and b == data, "the column must be one page holding exactly the script's output"
        got.append((info, stream))
        return stream
    raw = repack(write(t, **kw), fn)
    assert len(got) == 1
    return Forged(t, raw, got, damaged_from is not None)


def forge_pages(t: pa.Table, make: Callable[[PageInfo, bytes], object], **kw) -> Forged:
    """every page of `t` as pyarrow writes it, re-compressed by make(info, inflated) (checked by the strict decoder)"""
    got = []

    def fn(info, b):
        s = make(info, b)
        if s is not None and not isinstance(s, Stored):
            assert decode(s, expect=len(b))[0] == b
            got.append((info, s))
        return s
    return Forged(t, repack(write(t, **kw), fn), got)


def respeller(seed: int, pre: Optional[int] = None, **mix):
    rng = np.random.default_rng(seed)

    def make(info, b):
        p = pre if pre is None or len(varint(len(b))) <= pre else None
        return encode(respell(canonical(b), rng, **mix), preamble=p)
    return make
