"""Forged Arrow IPC streams (pure Python + numpy + pyarrow, no GPU, no flatbuffers package).

pyarrow's writer emits one shape of stream: V5 metadata behind a continuation marker, buffers 64-byte aligned in schema order,
exact lengths, clean padding bits, honest counts.  The format allows much more, and `chq_record_from_ipc` (csrc/ipc.cpp) takes
its bytes from another process, so it has to survive everything.  This module writes any stream from a description:

  Builder / Reader          a back-to-front flatbuffer builder (tables with fields in any order and vtables longer than the
                            known fields, strings, offset vectors, vectors of (int64, int64) structs and of int64) and a strict
                            reader that refuses every offset that leaves the buffer
  Field / Batch / Extra / Stream   the description: schema, record-batch messages with their bodies, other messages, framing
  describe                  a pyarrow batch (or the bytes of a stream) -> Stream
  build / build_messages / header_and_body   Stream -> bytes
  buffer_bytes / lay_out    the buffers of a batch message, and a body laid out with chosen offsets, gaps, filler, junk behind
                            the buffers, shared buffers and trailing bytes
Flatbuffer field ids are those of arrow/format/Schema.fbs and Message.fbs."""
from __future__ import annotations

import struct
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple, Union

import pyarrow as pa

# Type union tags (Schema.fbs)
(NONE, NULL, INT, FLOAT, BINARY, UTF8, BOOL, DECIMAL, DATE, TIME, TIMESTAMP, INTERVAL, LIST, STRUCT, UNION, FSB, FSL, MAP,
 DURATION, LARGEBINARY, LARGEUTF8, LARGELIST, REE, BINARYVIEW, UTF8VIEW) = range(25)
# MessageHeader union tags (Message.fbs)
SCHEMA, DICTIONARY_BATCH, RECORD_BATCH, TENSOR, SPARSE_TENSOR = 1, 2, 3, 4, 5
V4, V5 = 3, 4
LZ4_FRAME, ZSTD = 0, 1
CONTINUATION = b"\xff\xff\xff\xff"

# scalar / string fields of the type tables: tag -> [(field id, struct format or 's' for a string, default)]
TYPE_LAYOUT: Dict[int, List[Tuple[int, str, object]]] = {
    NULL: [], BINARY: [], UTF8: [], BOOL: [], LIST: [], STRUCT: [], LARGEBINARY: [], LARGEUTF8: [], LARGELIST: [], BINARYVIEW: [],
    UTF8VIEW: [],
    INT: [(0, "i", 0), (1, "?", False)],
    FLOAT: [(0, "h", 0)],
    DECIMAL: [(0, "i", 0), (1, "i", 0), (2, "i", 128)],
    DATE: [(0, "h", 1)],
    TIME: [(0, "h", 1), (1, "i", 32)],
    TIMESTAMP: [(0, "h", 0), (1, "s", None)],
    INTERVAL: [(0, "h", 0)],
    FSB: [(0, "i", 0)],
    FSL: [(0, "i", 0)],
    MAP: [(0, "?", False)],
    DURATION: [(0, "h", 1)],
}


class ForgeError(ValueError):
    """the strict reader met metadata that is not a well-formed flatbuffer / stream"""


# ---- flatbuffers: write ------------------------------------------------------------------------------------------------------
class Builder:
    """Back to front, like the reference implementation: children first (higher addresses).  A position is the distance of
    an object's first byte from the END of the buffer; `tail_pad` bytes of zeros (a multiple of 8) end the buffer."""

    def __init__(self, tail_pad: int = 0):
        assert tail_pad % 8 == 0
        self.b = bytearray(tail_pad)
        self.minalign = 1

    def size(self) -> int:
        return len(self.b)

    def _prepend(self, data: bytes) -> None:
        self.b[0:0] = data

    def pad(self, n: int) -> None:
        self._prepend(bytes(n))

    def align(self, a: int) -> None:
        self.minalign = max(self.minalign, a)
        self.pad(-self.size() % a)

    def prealign(self, length: int, a: int) -> None:
        self.minalign = max(self.minalign, a)
        self.pad(-(self.size() + length) % a)

    def push(self, fmt: str, v) -> int:
        self.align(struct.calcsize("<" + fmt))
        self._prepend(struct.pack("<" + fmt, v))
        return self.size()

    def string(self, s: Union[str, bytes], declared_len: Optional[int] = None) -> int:
        raw = s.encode() if isinstance(s, str) else bytes(s)
        self.prealign(len(raw) + 1, 4)
        self.pad(1)
        self._prepend(raw)
        return self.push("I", len(raw) if declared_len is None else declared_len)

    def offset_vector(self, targets: Sequence[int], declared_len: Optional[int] = None) -> int:
        self.prealign(4 * len(targets), 4)
        for t in reversed(targets):
            self.push("I", self.size() + 4 - t)
        return self.push("I", len(targets) if declared_len is None else declared_len)

    def pair_vector(self, pairs: Sequence[Tuple[int, int]], declared_len: Optional[int] = None) -> int:
        """[FieldNode] / [Buffer]: structs of two int64, 8-aligned behind the 4-byte element count"""
        self.prealign(16 * len(pairs), 8)
        for a, b in reversed(pairs):
            self._prepend(struct.pack("<qq", _wrap64(a), _wrap64(b)))
        return self.push("I", len(pairs) if declared_len is None else declared_len)

    def long_vector(self, values: Sequence[int]) -> int:
        self.prealign(8 * len(values), 8)
        for v in reversed(values):
            self._prepend(struct.pack("<q", v))
        return self.push("I", len(values))

    def table(self, fields: Sequence[Tuple[int, str, object]], extra_slots: int = 0) -> int:
        """fields: (field id, struct format or 'ref', value or target position), stored in the order given (the first at the
        highest address); a 'ref' without a target is left out.  `extra_slots` empty vtable entries follow the last id."""
        start = self.size()
        locs = {}
        for fid, fmt, v in fields:
            if fmt == "ref":
                if not v:
                    continue
                self.align(4)
                self.push("I", self.size() + 4 - v)
            else:
                self.push(fmt, _wrap64(v) if fmt == "q" else v)
            locs[fid] = self.size()
        self.align(4)
        table = self.push("i", 0)
        slots = max(locs, default=-1) + 1 + extra_slots
        vt = struct.pack("<HH", 4 + 2 * slots, table - start)
        vt += b"".join(struct.pack("<H", table - locs[i] if i in locs else 0) for i in range(slots))
        self._prepend(vt)
        self.b[len(self.b) - table:len(self.b) - table + 4] = struct.pack("<i", self.size() - table)
        return table

    def finish(self, root: int) -> bytes:
        self.prealign(4, max(self.minalign, 8))
        self.push("I", self.size() + 4 - root)
        return bytes(self.b)


def _wrap64(v: int) -> int:
    """forged values are given as Python ints; 2^63.. wrap to the int64 the wire holds"""
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >> 63 else v


# ---- flatbuffers: read -------------------------------------------------------------------------------------------------------
class Reader:
    """strict: every position is checked against the buffer"""

    def __init__(self, buf: bytes):
        self.b = bytes(buf)

    def rd(self, fmt: str, pos: int):
        n = struct.calcsize("<" + fmt)
        if pos < 0 or pos + n > len(self.b):
            raise ForgeError(f"read of {n} bytes at {pos} outside {len(self.b)}")
        return struct.unpack_from("<" + fmt, self.b, pos)[0]

    def follow(self, pos: int) -> int:
        o = self.rd("I", pos)
        if o == 0 or pos + o >= len(self.b):
            raise ForgeError(f"offset {o} at {pos}")
        return pos + o

    def root(self) -> int:
        return self.follow(0)

    def vtable(self, t: int) -> Tuple[int, int, int]:
        vt = t - self.rd("i", t)
        size, tsize = self.rd("H", vt), self.rd("H", vt + 2)
        if size < 4 or size % 2 or vt + size > len(self.b) or tsize < 4 or t + tsize > len(self.b):
            raise ForgeError(f"vtable at {vt}: size {size}, table size {tsize}")
        return vt, size, tsize

    def slots(self, t: int) -> int:
        return (self.vtable(t)[1] - 4) // 2

    def field(self, t: int, fid: int) -> Optional[int]:
        vt, size, tsize = self.vtable(t)
        if 4 + 2 * fid + 2 > size:
            return None
        off = self.rd("H", vt + 4 + 2 * fid)
        if off == 0:
            return None
        if off < 4 or off >= tsize:
            raise ForgeError(f"field {fid} at offset {off} of a {tsize}-byte table")
        return t + off

    def scalar(self, t: int, fid: int, fmt: str, default):
        p = self.field(t, fid)
        return default if p is None else self.rd(fmt, p)

    def ref(self, t: int, fid: int) -> Optional[int]:
        p = self.field(t, fid)
        return None if p is None else self.follow(p)

    def string_at(self, s: int) -> str:
        n = self.rd("I", s)
        if s + 4 + n > len(self.b):
            raise ForgeError(f"string of {n} bytes at {s}")
        return self.b[s + 4:s + 4 + n].decode()

    def string(self, t: int, fid: int) -> Optional[str]:
        s = self.ref(t, fid)
        return None if s is None else self.string_at(s)

    def vector(self, t: int, fid: int, elem: int) -> Tuple[Optional[int], int]:
        """(position of the first element, count)"""
        v = self.ref(t, fid)
        if v is None:
            return None, 0
        n = self.rd("I", v)
        if v + 4 + n * elem > len(self.b):
            raise ForgeError(f"vector of {n} x {elem} bytes at {v}")
        return v + 4, n

    def tables(self, t: int, fid: int) -> List[int]:
        p, n = self.vector(t, fid, 4)
        return [self.follow(p + 4 * i) for i in range(n)]

    def key_values(self, t: int, fid: int) -> List[Tuple[str, str]]:
        return [(self.string(kv, 0) or "", self.string(kv, 1) or "") for kv in self.tables(t, fid)]


# ---- the description ---------------------------------------------------------------------------------------------------------
@dataclass
class Field:
    name: str
    nullable: bool
    type_tag: int
    type_fields: List[Tuple[int, str, object]] = field(default_factory=list)   # (id, struct format or 's', value)
    children: List["Field"] = field(default_factory=list)
    dictionary: Optional[dict] = None          # {"id", "index": (bitWidth, signed), "ordered"}
    metadata: List[Tuple[str, str]] = field(default_factory=list)
    extra_slots: int = 0


@dataclass
class Batch:
    """one RecordBatch message and its body"""
    length: int
    nodes: List[Tuple[int, int]]               # (length, null_count) per field, depth first
    buffers: List[Tuple[int, int]]             # (offset, length) into the body
    body: bytes = b""
    body_length: Optional[int] = None          # what the message says; None: len(body)
    compression: Optional[Tuple[int, int]] = None   # (codec, method)
    variadic: Optional[List[int]] = None       # variadicBufferCounts
    metadata: List[Tuple[str, str]] = field(default_factory=list)   # the message's custom_metadata
    extra_slots: int = 0                       # empty vtable entries behind the known fields of the RecordBatch table


@dataclass
class Extra:
    """a message of any other kind; header_table=False leaves the header union empty"""
    header_type: int
    body_length: int = 0
    body: bytes = b""
    header_table: bool = True


@dataclass
class Stream:
    fields: List[Field]
    messages: List[Union[Batch, Extra]] = field(default_factory=list)
    endianness: int = 0
    metadata: List[Tuple[str, str]] = field(default_factory=list)           # the schema's custom_metadata
    message_metadata: List[Tuple[str, str]] = field(default_factory=list)   # the schema MESSAGE's custom_metadata
    schema_at: Optional[int] = 0               # index among `messages` before which the schema message goes; None: no schema
    legacy_framing: bool = False               # pre-0.15: a 4-byte size without the continuation marker, 4-byte end marker
    version: int = V5
    eos: bool = True
    meta_pad: int = 0                          # zero bytes (a multiple of 8) behind every metadata flatbuffer
    tail_pad: int = 0                          # zero bytes (a multiple of 8) inside every flatbuffer, at its end
    extra_slots: int = 0                       # empty vtable entries behind the known fields of Message and Schema tables

    @property
    def batch(self) -> Batch:
        return next(m for m in self.messages if isinstance(m, Batch))


# ---- Stream -> bytes ---------------------------------------------------------------------------------------------------------
def _key_values(b: Builder, kvs) -> int:
    if not kvs:
        return 0
    tables = []
    for k, v in kvs:
        ks, vs = b.string(k), b.string(v)
        tables.append(b.table([(0, "ref", ks), (1, "ref", vs)]))
    return b.offset_vector(tables)


def _type_table(b: Builder, f: Field) -> int:
    strings = {fid: b.string(v) for fid, fmt, v in f.type_fields if fmt == "s" and v is not None}
    return b.table([(fid, "ref", strings.get(fid)) if fmt == "s" else (fid, fmt, v) for fid, fmt, v in f.type_fields])


def _field_table(b: Builder, f: Field) -> int:
    children = b.offset_vector([_field_table(b, c) for c in f.children])
    kv = _key_values(b, f.metadata)
    dic = 0
    if f.dictionary is not None:
        idx = b.table([(0, "i", f.dictionary["index"][0]), (1, "?", f.dictionary["index"][1])])
        dic = b.table([(0, "q", f.dictionary["id"]), (1, "ref", idx), (2, "?", f.dictionary.get("ordered", False))])
    ty = _type_table(b, f)
    name = b.string(f.name)
    return b.table([(0, "ref", name), (1, "?", f.nullable), (2, "B", f.type_tag), (3, "ref", ty), (4, "ref", dic), (5, "ref", children),
                    (6, "ref", kv)], f.extra_slots)


def _message(s: Stream, header_type: int, header: Optional[int], body_length: int, b: Builder, kvs=()) -> bytes:
    kv = _key_values(b, kvs)
    root = b.table([(0, "h", s.version), (1, "B", header_type), (2, "ref", header), (3, "q", body_length), (4, "ref", kv)], s.extra_slots)
    return b.finish(root)


def schema_flatbuffer(s: Stream) -> bytes:
    b = Builder(s.tail_pad)
    fields = b.offset_vector([_field_table(b, f) for f in s.fields])
    kv = _key_values(b, s.metadata)
    schema = b.table([(0, "h", s.endianness), (1, "ref", fields), (2, "ref", kv)], s.extra_slots)
    return _message(s, SCHEMA, schema, 0, b, s.message_metadata)


def message_flatbuffer(s: Stream, m: Union[Batch, Extra]) -> bytes:
    b = Builder(s.tail_pad)
    if isinstance(m, Extra):
        return _message(s, m.header_type, b.table([]) if m.header_table else None, m.body_length, b)
    variadic = b.long_vector(m.variadic) if m.variadic is not None else 0
    comp = b.table([(0, "b", m.compression[0]), (1, "b", m.compression[1])]) if m.compression is not None else 0
    buffers = b.pair_vector(m.buffers)
    nodes = b.pair_vector(m.nodes)
    rb = b.table([(0, "q", m.length), (1, "ref", nodes), (2, "ref", buffers), (3, "ref", comp), (4, "ref", variadic)], m.extra_slots)
    return _message(s, RECORD_BATCH, rb, len(m.body) if m.body_length is None else m.body_length, b, m.metadata)


def frame(s: Stream, fb: bytes) -> bytes:
    """the size prefix and the metadata, padded so that the body starts 8-aligned"""
    prefix = 4 if s.legacy_framing else 8
    size = len(fb) + (-(prefix + len(fb)) % 8) + s.meta_pad
    return (b"" if s.legacy_framing else CONTINUATION) + struct.pack("<i", size) + fb + bytes(size - len(fb))


def build_messages(s: Stream) -> List[Tuple[bytes, bytes]]:
    """[(framed metadata, body)] in stream order, without the end-of-stream marker"""
    out = [(frame(s, message_flatbuffer(s, m)), bytes(m.body)) for m in s.messages]
    if s.schema_at is not None:
        out.insert(s.schema_at, (frame(s, schema_flatbuffer(s)), b""))
    return out


def end_marker(s: Stream) -> bytes:
    return bytes(4) if s.legacy_framing else CONTINUATION + bytes(4)


def build(s: Stream) -> bytes:
    return b"".join(meta + body for meta, body in build_messages(s)) + (end_marker(s) if s.eos else b"")


def header_and_body(s: Stream) -> Tuple[bytes, bytes]:
    """the metadata part -- every message up to and including the first batch's metadata -- and that batch's body: what a
    sender that moves the body on its own passes"""
    header = b""
    for (meta, body), m in zip(build_messages(s), _with_schema(s)):
        header += meta
        if isinstance(m, Batch):
            return header, body
        header += body
    raise ValueError("no batch message")


def _with_schema(s: Stream) -> list:
    out = list(s.messages)
    if s.schema_at is not None:
        out.insert(s.schema_at, None)
    return out


# ---- bytes -> Stream ---------------------------------------------------------------------------------------------------------
def split_messages(stream: bytes) -> Tuple[List[Tuple[int, int, int]], bool, bool]:
    """([(metadata position, metadata size, body position)], legacy framing, end marker seen): the framing alone; the body
    length comes from each message's metadata"""
    at, out, legacy, eos = 0, [], False, False
    while at + 4 <= len(stream):
        first = stream[at:at + 4]
        if first == CONTINUATION:
            if at + 8 > len(stream):
                raise ForgeError("continuation marker without a size")
            size, at = struct.unpack_from("<i", stream, at + 4)[0], at + 8
        else:
            size, at, legacy = struct.unpack_from("<i", stream, at)[0], at + 4, True
        if size == 0:
            eos = True
            break
        if size < 0 or at + size > len(stream):
            raise ForgeError(f"message of {size} bytes at {at}")
        r = Reader(stream[at:at + size])
        body_len = r.scalar(r.root(), 3, "q", 0)
        if body_len < 0 or at + size + body_len > len(stream):
            raise ForgeError(f"body of {body_len} bytes at {at + size}")
        out.append((at, size, at + size))
        at += size + body_len
    return out, legacy, eos


def _read_field(r: Reader, t: int) -> Field:
    tag = r.scalar(t, 2, "B", 0)
    if tag not in TYPE_LAYOUT:
        raise ForgeError(f"type tag {tag}")
    ty = r.ref(t, 3)
    if ty is None:
        raise ForgeError("field without a type table")
    type_fields = []
    for fid, fmt, default in TYPE_LAYOUT[tag]:
        if fmt == "s":
            v = r.string(ty, fid)
            if v is not None:
                type_fields.append((fid, "s", v))
        else:
            type_fields.append((fid, fmt, r.scalar(ty, fid, fmt, default)))
    dic = None
    d = r.ref(t, 4)
    if d is not None:
        idx = r.ref(d, 1)
        dic = {"id": r.scalar(d, 0, "q", 0), "index": (r.scalar(idx, 0, "i", 0), r.scalar(idx, 1, "?", False)) if idx is not None else (32, True),
               "ordered": r.scalar(d, 2, "?", False)}
    return Field(r.string(t, 0) or "", r.scalar(t, 1, "?", False), tag, type_fields, [_read_field(r, c) for c in r.tables(t, 5)], dic,
                 r.key_values(t, 6))


def describe(rec_or_stream: Union[pa.RecordBatch, bytes]) -> Stream:
    stream = rec_or_stream
    if isinstance(stream, pa.RecordBatch):
        sink = pa.BufferOutputStream()
        with pa.ipc.new_stream(sink, stream.schema) as w:
            w.write_batch(stream)
        stream = sink.getvalue().to_pybytes()
    frames, legacy, eos = split_messages(stream)
    out = Stream(fields=[], schema_at=None, legacy_framing=legacy, eos=eos)
    for at, size, body_at in frames:
        r = Reader(stream[at:at + size])
        m = r.root()
        out.version = r.scalar(m, 0, "h", 0)
        htype, h, body_len = r.scalar(m, 1, "B", 0), r.ref(m, 2), r.scalar(m, 3, "q", 0)
        body = stream[body_at:body_at + body_len]
        if htype == SCHEMA and h is not None:
            if out.schema_at is not None:
                raise ForgeError("two schema messages")
            out.schema_at = len(out.messages)
            out.endianness = r.scalar(h, 0, "h", 0)
            out.fields = [_read_field(r, f) for f in r.tables(h, 1)]
            out.metadata = r.key_values(h, 2)
            out.message_metadata = r.key_values(m, 4)
        elif htype == RECORD_BATCH and h is not None:
            def pairs(fid):
                p, n = r.vector(h, fid, 16)
                return [(r.rd("q", p + 16 * i), r.rd("q", p + 16 * i + 8)) for i in range(n)]
            comp = r.ref(h, 3)
            vp, vn = r.vector(h, 4, 8)
            out.messages.append(Batch(r.scalar(h, 0, "q", 0), pairs(1), pairs(2), body, None,
                                      None if comp is None else (r.scalar(comp, 0, "b", 0), r.scalar(comp, 1, "b", 0)),
                                      None if vp is None else [r.rd("q", vp + 8 * i) for i in range(vn)], r.key_values(m, 4)))
        else:
            out.messages.append(Extra(htype, body_len, body, h is not None))
    return out


# ---- bodies ------------------------------------------------------------------------------------------------------------------
def buffer_bytes(b: Batch) -> List[bytes]:
    return [bytes(b.body[off:off + ln]) for off, ln in b.buffers]


def lay_out(bufs: Sequence[bytes], *, order: Optional[Sequence[int]] = None, align: int = 8, lead: int = 0, gap: int = 0,
            filler: int = 0xA5, slack: int = 0, share: Optional[Dict[int, int]] = None, trailing: int = 0) -> Tuple[bytes, List[Tuple[int, int]]]:
    """A body holding `bufs`, placed in `order` (indices; default: as given), each at a multiple of `align`, `lead` filler bytes
    first and at least `gap` between two buffers.  Every buffer is DECLARED `slack` bytes longer than its content, with filler
    behind it.  share[j] = i gives buffer j the very (offset, length) of buffer i (its own bytes are not stored).  `trailing`
    filler bytes end the body, which is padded to a multiple of 8.  Returns (body, [(offset, length)] in the order of `bufs`)."""
    share = share or {}
    body = bytearray([filler]) * lead
    table: List[Optional[Tuple[int, int]]] = [None] * len(bufs)
    for i in (order if order is not None else range(len(bufs))):
        if i in share:
            continue
        body += bytes([filler]) * (-len(body) % align)
        table[i] = (len(body), len(bufs[i]) + slack)
        body += bufs[i] + bytes([filler]) * (slack + gap)
    for j, i in share.items():
        table[j] = table[i]
    body += bytes([filler]) * trailing
    body += bytes([filler]) * (-len(body) % 8)
    return bytes(body), table   # type: ignore[return-value]


def relaid(s: Stream, **how) -> Stream:
    """`s` with its batch's body laid out again (see lay_out); `s` itself is changed and returned"""
    b = s.batch
    b.body, b.buffers = lay_out(buffer_bytes(b), **how)
    return s


def read_back(stream: bytes) -> pa.RecordBatch:
    """what pyarrow reads from a one-batch stream, fully validated"""
    reader = pa.ipc.open_stream(stream)
    batches = list(reader)
    assert len(batches) <= 1
    rec = batches[0] if batches else pa.RecordBatch.from_pylist([], schema=reader.schema)
    rec.validate(full=True)
    return rec
