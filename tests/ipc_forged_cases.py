"""The forged Arrow IPC streams of tests/test_ipc_forge.py (pyarrow reads the legal ones as declared) and
tests/test_ipc_forged.py (csrc/ipc.cpp reads the legal ones like pyarrow and refuses the others).  Pure Python + numpy + pyarrow.

  legal_cases()          {id: (stream bytes, the batch the case DECLARES)}     -- group A
  out_of_scope_cases()   {id: (stream bytes, the word the message must hold)}  -- group B, CHQ_ERR_NOT_SUPPORTED
  illegal_cases()        {id: stream bytes}                                    -- group C, refused from the metadata alone
  type_table_cases()     {id: stream bytes}                                    -- group C.9, refused with 22 or 30
  skipped_message_cases(), damaged_flatbuffers(), mutated_streams(), run_sweep(), bad_offsets()"""
from __future__ import annotations

import copy
import datetime
import decimal
import functools
import struct
import sys

import numpy as np
import pyarrow as pa

from tests import ipc_forge as F

I63 = 2**63


def pyarrow_stream(rec: pa.RecordBatch) -> bytes:
    sink = pa.BufferOutputStream()
    with pa.ipc.new_stream(sink, rec.schema) as w:
        w.write_batch(rec)
    return sink.getvalue().to_pybytes()


# ---- type coverage (A.8): written by pyarrow ---------------------------------------------------------------------------------
COVERAGE_TYPES = (
    [pa.int8(), pa.int16(), pa.int32(), pa.int64(), pa.uint8(), pa.uint16(), pa.uint32(), pa.uint64(), pa.float16(), pa.float32(),
     pa.float64(), pa.bool_(), pa.utf8(), pa.date32(), pa.date64(), pa.time32("s"), pa.time32("ms"), pa.time64("us"), pa.time64("ns")]
    + [pa.timestamp(u, tz=tz) for u in ("s", "ms", "us", "ns") for tz in (None, "UTC", "+02:00")]
    + [pa.duration(u) for u in ("s", "ms", "us", "ns")]
    + [pa.decimal128(1, 0), pa.decimal128(20, 2), pa.decimal128(38, 10), pa.decimal128(38, -3)]
    + [pa.binary(1), pa.binary(3), pa.binary(16)])


def random_array(rng, t: pa.DataType, n: int, nulls: bool) -> pa.Array:
    """n values of type t from raw buffers (every bit pattern that is a legal value of t), every fifth row null with `nulls`"""
    valid = np.ones(n, bool)
    if nulls:
        valid[rng.random(n) < 0.2] = False
    count = int((~valid).sum())
    bitmap = pa.py_buffer(np.packbits(valid, bitorder="little").tobytes()) if count else None
    if pa.types.is_string(t):
        lengths = rng.integers(0, 9, n)
        offs = np.zeros(n + 1, np.int32)
        np.cumsum(lengths, out=offs[1:])
        data = rng.integers(ord("a"), ord("z") + 1, int(offs[-1])).astype(np.uint8)
        bufs = [bitmap, pa.py_buffer(offs.tobytes()), pa.py_buffer(data.tobytes())]
    elif pa.types.is_boolean(t):
        bufs = [bitmap, pa.py_buffer(np.packbits(rng.random(n) < 0.5, bitorder="little").tobytes())]
    elif pa.types.is_decimal(t):
        digits = [int(rng.integers(0, 10**9)) * 10**29 + int(rng.integers(0, 10**18)) for _ in range(n)]
        vals = [(d % 10**t.precision) * (1 if i % 2 else -1) for i, d in enumerate(digits)]
        bufs = [bitmap, pa.py_buffer(b"".join(v.to_bytes(16, "little", signed=True) for v in vals))]
    elif pa.types.is_date64(t):
        bufs = [bitmap, pa.py_buffer((rng.integers(-10**4, 10**5, n) * 86_400_000).astype(np.int64).tobytes())]
    elif pa.types.is_time(t):
        per_day = {"s": 86_400, "ms": 86_400_000, "us": 86_400_000_000, "ns": 86_400_000_000_000}[t.unit]
        bufs = [bitmap, pa.py_buffer(rng.integers(0, per_day, n).astype(np.int32 if t.bit_width == 32 else np.int64).tobytes())]
    elif pa.types.is_float16(t):
        bufs = [bitmap, pa.py_buffer(rng.integers(0, 2**16, n).astype(np.uint16).tobytes())]
    else:
        width = t.byte_width
        bufs = [bitmap, pa.py_buffer(rng.integers(0, 256, n * width).astype(np.uint8).tobytes())]
    arr = pa.Array.from_buffers(t, n, bufs, null_count=count)
    arr.validate(full=True)
    return arr


def coverage_batch(n: int, seed: int = 0) -> pa.RecordBatch:
    """one column per type of COVERAGE_TYPES, nulls in every second column"""
    rng = np.random.default_rng(seed)
    arrays = [random_array(rng, t, n, nulls=(i % 2 == 1)) for i, t in enumerate(COVERAGE_TYPES)]
    fields = [pa.field(f"c{i}", t, nullable=True) for i, t in enumerate(COVERAGE_TYPES)]
    return pa.RecordBatch.from_arrays(arrays, schema=pa.schema(fields))


# ---- the base batch of the forged cases --------------------------------------------------------------------------------------
def base_batch(n: int = 65, seed: int = 1) -> pa.RecordBatch:
    """x Int32 (nulls), flag Boolean (nulls), s Utf8 (nulls), f Float64; buffers: 0 1 | 2 3 | 4 5 6 | 7 8"""
    rng = np.random.default_rng(seed)
    mask = lambda: (np.arange(n) % 5 == int(rng.integers(0, 5))) if n > 1 else np.zeros(n, bool)   # noqa: E731
    words = np.array(["", "a", "bc", "héllo", "0123456789abcdef"], dtype=object)
    return pa.RecordBatch.from_arrays(
        [pa.array(rng.integers(-1000, 1000, n).astype(np.int32), mask=mask()),
         pa.array(rng.random(n) < 0.5, mask=mask()),
         pa.array(words[rng.integers(0, len(words), n)], type=pa.utf8(), mask=mask()),
         pa.array(rng.random(n))],
        schema=pa.schema([pa.field("x", pa.int32()), pa.field("flag", pa.bool_()), pa.field("s", pa.utf8()), pa.field("f", pa.float64(), nullable=False)]))


BUF = {"validity": 0, "values": 1, "bitmap": 3, "offsets": 5}   # one buffer of each kind in base_batch


def stream_of(schema: pa.Schema, n: int, nodes, bufs, **layout) -> F.Stream:
    """a stream of `schema` whose one batch has these nodes and buffers (bytes), laid out by ipc_forge.lay_out"""
    s = F.describe(pa.RecordBatch.from_pylist([], schema=schema))
    body, table = F.lay_out(bufs, **layout)
    s.messages = [F.Batch(n, list(nodes), table, body)]
    return s


def junk_padding(bitmap: bytes, n: int) -> bytes:
    """every bit past the first n set"""
    b = bytearray(bitmap)
    for i in range(n, 8 * len(b)):
        b[i >> 3] |= 1 << (i & 7)
    return bytes(b)


# ---- A: legal streams no pyarrow writer emits --------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def legal_cases() -> dict:
    out = {}
    rec = base_batch()
    n = rec.num_rows
    # 1. framing and metadata version
    for name, how in [("legacy-framing", dict(legacy_framing=True)), ("v4", dict(version=F.V4)), ("legacy-v4", dict(legacy_framing=True, version=F.V4)),
                      ("no-end-marker", dict(eos=False))]:
        s = F.describe(rec)
        for k, v in how.items():
            setattr(s, k, v)
        out[name] = (F.build(s), rec)
    # 2. body layout: 8- but not 64-aligned, shuffled, 0xA5 between the buffers, declared longer than needed, junk behind
    s = F.relaid(F.describe(rec), order=[8, 3, 0, 6, 5, 1, 7, 2, 4], align=8, lead=8, gap=3, slack=13, trailing=21)
    assert all(off % 8 == 0 for off, _ in s.batch.buffers) and any(off % 64 for off, _ in s.batch.buffers)
    out["shuffled-body"] = (F.build(s), rec)
    twins = pa.RecordBatch.from_arrays([rec.column(0), rec.column(0), rec.column(3)], names=["a", "b", "f"])
    s = F.relaid(F.describe(twins), lead=8, share={3: 1, 2: 0})     # b's validity and values ARE a's
    assert s.batch.buffers[3] == s.batch.buffers[1]
    out["shared-values-buffer"] = (F.build(s), twins)
    # 3. a validity buffer with zero bits next to null_count 0: dropped, every row valid
    s = F.describe(rec)
    bufs = F.buffer_bytes(s.batch)
    assert bufs[0] and rec.column(0).null_count
    s.batch.nodes[0] = (n, 0)
    all_valid = pa.Array.from_buffers(pa.int32(), n, [None, pa.py_buffer(bufs[1])])
    out["validity-with-null-count-0"] = (F.build(s), pa.RecordBatch.from_arrays([all_valid] + rec.columns[1:], schema=rec.schema))
    # 4. a validity buffer of length 0 with null_count 0, placed at the very end of the body
    plain = pa.RecordBatch.from_arrays([rec.column(3), pa.array(np.arange(n, dtype=np.int64))], names=["f", "k"])
    s = F.describe(plain)
    assert s.batch.buffers[0][1] == 0 and s.batch.buffers[2][1] == 0
    s.batch.buffers[0] = (len(s.batch.body), 0)
    out["empty-validity"] = (F.build(s), plain)
    # 5. junk in the padding bits of validity and Boolean buffers
    for k in (1, 7, 63, 65):
        out[f"padding-junk-{k}"] = padding_junk_case(k)
    # 6. Utf8 layouts
    out.update(utf8_layout_cases())
    # 7. a vtable that carries an empty variadicBufferCounts, custom metadata everywhere, padded metadata, long vtables
    s = F.describe(rec)
    s.batch.variadic = []
    s.batch.metadata = [("batch", "meta")]
    s.batch.extra_slots = 2
    s.metadata = [("schema", "meta"), ("k", "")]
    s.message_metadata = [("message", "meta")]
    s.fields[1].metadata = [("field", "meta")]
    s.fields[2].extra_slots = 3
    s.meta_pad, s.tail_pad, s.extra_slots = 24, 16, 4
    fields = [rec.schema.field(i) for i in range(4)]
    fields[1] = fields[1].with_metadata({"field": "meta"})
    declared = pa.RecordBatch.from_arrays(rec.columns, schema=pa.schema(fields, metadata={"schema": "meta", "k": ""}))
    out["metadata-everywhere"] = (F.build(s), declared)
    return out


def padding_junk_case(n: int):
    rec = base_batch(n, seed=40 + n)
    s = F.describe(rec)
    bufs = F.buffer_bytes(s.batch)
    for i in (0, 2, 3, 4):
        bufs[i] = junk_padding(bufs[i], n)
    s.batch.body, s.batch.buffers = F.lay_out(bufs)
    return F.build(s), rec


def utf8_layout_cases() -> dict:
    out = {}
    schema = pa.schema([pa.field("s", pa.utf8()), pa.field("k", pa.int32(), nullable=False)])

    def case(strings, offs, data, valid=None, offsets_buf=None):
        n = len(strings)
        nulls = 0 if valid is None else int((~valid).sum())
        vbuf = np.packbits(valid, bitorder="little").tobytes() if nulls else b""
        obuf = np.asarray(offs, np.int32).tobytes() if offsets_buf is None else offsets_buf
        s = stream_of(schema, n, [(n, nulls), (n, 0)], [vbuf, obuf, data, b"", np.arange(n, dtype=np.int32).tobytes()], lead=8, gap=5)
        declared = pa.RecordBatch.from_arrays([pa.array(strings, type=pa.utf8()), pa.array(np.arange(n, dtype=np.int32))], schema=schema)
        return F.build(s), declared
    words = ["alpha", "", "βeta", None, "gamma-gamma-gamma", "", "z"]
    raw = [(w or "").encode() for w in words]
    ends = np.cumsum([len(r) for r in raw])
    valid = np.array([w is not None for w in words])
    out["utf8-first-offset-nonzero"] = case(words, np.concatenate([[11], 11 + ends]), b"\xff" * 11 + b"".join(raw) + b"\xfe" * 9, valid)
    out["utf8-all-empty-no-data"] = case([""] * 9, np.zeros(10), b"")
    tail = ["ab", "cde", "", "", ""]
    out["utf8-trailing-empty-at-data-end"] = case(tail, [0, 2, 5, 5, 5, 5], b"abcde")
    out["utf8-zero-rows-no-offsets"] = case([], [], b"", offsets_buf=b"")
    return out


# ---- B: legal but out of scope -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def out_of_scope_cases() -> dict:
    out = {}

    def one(arr):
        return pyarrow_stream(pa.RecordBatch.from_arrays([arr], names=["c"]))
    out["LargeUtf8"] = (one(pa.array(["a", None], type=pa.large_utf8())), "LargeUtf8")
    out["Binary"] = (one(pa.array([b"a", None], type=pa.binary())), "Binary")
    out["Null"] = (one(pa.nulls(3)), "Null")
    out["Interval"] = (one(pa.array([None, None], type=pa.month_day_nano_interval())), "Interval")
    out["Decimal256"] = (one(pa.array([decimal.Decimal("1.5"), None], type=pa.decimal256(40, 2))), "Decimal256")
    dec = pa.RecordBatch.from_arrays([pa.array([decimal.Decimal("1.5"), None], type=pa.decimal128(9, 2))], names=["c"])
    for bits in (32, 64):
        s = F.describe(dec)
        s.fields[0].type_fields = [(0, "i", 9), (1, "i", 2), (2, "i", bits)]
        out[f"Decimal{bits}"] = (F.build(s), f"Decimal{bits}")
    s = F.describe(pa.RecordBatch.from_arrays([pa.array(["a", None])], names=["c"]))
    s.fields[0].type_tag = F.UTF8VIEW
    s.batch.variadic = [0]
    out["Utf8View"] = (F.build(s), "Utf8View")
    out["Struct"] = (one(pa.array([{"a": 1}, None])), "nested")
    out["List"] = (one(pa.array([[1, 2], [3]])), "nested")
    out["dictionary-field"] = (one(pa.array(["a", "b", "a"]).dictionary_encode()), "dictionary")
    for codec, name in ((F.LZ4_FRAME, "LZ4"), (F.ZSTD, "ZSTD")):
        s = F.describe(base_batch())
        s.batch.compression = (codec, 0)
        out[f"compression-{name}"] = (F.build(s), name)
    s = F.describe(base_batch())
    s.endianness = 1
    out["big-endian"] = (F.build(s), "big-endian")
    s = F.describe(base_batch())
    s.messages.insert(0, F.Extra(F.DICTIONARY_BATCH, 0))
    out["dictionary-batch"] = (F.build(s), "dictionary")
    return out


# ---- C: illegal streams that the metadata alone gives away -------------------------------------------------------------------
def need_of(kind: str, n: int) -> int:
    return {"validity": (n + 7) // 8, "values": 4 * n, "bitmap": (n + 7) // 8, "offsets": 4 * (n + 1)}[kind]


@functools.lru_cache(maxsize=None)
def illegal_cases() -> dict:
    out = {}
    rec = base_batch()
    n = rec.num_rows
    base = F.describe(rec)
    body_len = len(base.batch.body)

    def forged(change) -> bytes:
        s = copy.deepcopy(base)
        change(s)
        return F.build(s)

    def set_buffer(i, pair):
        def change(s):
            s.batch.buffers[i] = pair
        return change
    # 1. buffer (offset, length) pairs, for each kind of buffer
    for kind, i in BUF.items():
        off, need = base.batch.buffers[i][0], need_of(kind, n)
        pairs = {"wrap-16": (I63 - 8, 16), "wrap-need": (I63 - 512, 512), "negative-offset": (-8, 8), "negative-length": (0, -1),
                 "past-body-end": (body_len - 4, 8), "one-short": (off, need - 1)}
        for name, pair in pairs.items():
            out[f"buffer-{kind}-{name}"] = forged(set_buffer(i, pair))
    # 2. row count and nodes
    for name, rows in [("minus-1", -1), ("2^61", 2**61), ("2^62", 2**62), ("2^63-1", I63 - 1)]:
        def change(s, rows=rows):
            s.batch.length = rows
            s.batch.nodes = [(rows, 0 if rows < 0 else nc) for _, nc in s.batch.nodes]
        out[f"rows-{name}"] = forged(change)

        def change0(s, rows=rows):   # without null counts: no validity to size, so n * width / (n + 1) * 4 / (n + 7) / 8 alone decide
            s.batch.length = rows
            s.batch.nodes = [(rows, 0) for _ in s.batch.nodes]
        out[f"rows-{name}-no-nulls"] = forged(change0)
    out["node-length-differs"] = forged(lambda s: s.batch.nodes.__setitem__(1, (n - 1, s.batch.nodes[1][1])))
    out["node-missing"] = forged(lambda s: s.batch.nodes.pop())
    out["node-extra"] = forged(lambda s: s.batch.nodes.append((n, 0)))
    out["too-few-buffers"] = forged(lambda s: s.batch.buffers.pop())
    # 3. null counts
    for name, nc in [("minus-1", -1), ("n+1", n + 1), ("2^63-1", I63 - 1)]:
        for col in (0, 1, 2):
            out[f"null-count-{name}-col{col}"] = forged(lambda s, nc=nc, col=col: s.batch.nodes.__setitem__(col, (n, nc)))
    # 4. bodyLength
    out["body-length-minus-1"] = forged(lambda s: setattr(s.batch, "body_length", -1))
    out["body-length-2^63-1"] = forged(lambda s: setattr(s.batch, "body_length", I63 - 1))
    last_end = max(off + ln for off, ln in base.batch.buffers)
    out["body-length-below-buffers"] = forged(lambda s: setattr(s.batch, "body_length", last_end - 8))
    # 5. framing
    good = F.build(base)
    out["negative-message-size"] = good[:4] + struct.pack("<i", -8) + good[8:]
    out["message-size-beyond-stream"] = good[:4] + struct.pack("<i", len(good)) + good[8:]
    out["legacy-message-size-beyond-stream"] = struct.pack("<i", len(good)) + good[8:]
    out["end-marker-first"] = F.CONTINUATION + bytes(4) + good
    out["schema-only"] = forged(lambda s: s.messages.clear())
    out["batch-before-schema"] = forged(lambda s: setattr(s, "schema_at", 1))
    out["no-schema"] = forged(lambda s: setattr(s, "schema_at", None))
    # 7. two record batches in one stream (the reference: ExchangeRequestsError::ReceivedMultipleRecordBatches)
    out["two-batches"] = forged(lambda s: s.messages.append(copy.deepcopy(s.messages[0])))
    out["two-batches-skipped-between"] = forged(lambda s: s.messages.extend([F.Extra(F.TENSOR, 8, bytes(8)), copy.deepcopy(s.messages[0])]))
    return out


def two_batch_header_and_body():
    """the metadata of TWO batches behind the schema, and one body: what a separate-body sender would pass"""
    s = F.describe(base_batch())
    parts = F.build_messages(s)
    return parts[0][0] + parts[1][0] + parts[1][0], parts[1][1]


# 6. messages of a kind the parser steps over, whose bodyLength leads the cursor astray
@functools.lru_cache(maxsize=None)
def skipped_message_cases() -> dict:
    out = {}
    for kind, extra in [("tensor", F.Extra(F.TENSOR)), ("no-header", F.Extra(0, header_table=False))]:
        s = F.describe(base_batch())
        s.messages.insert(0, extra)
        meta = len(F.build_messages(s)[1][0]) - 8
        total = len(F.build(s))
        for name, blen in [("back-to-itself", -(meta + 8)), ("minus-1", -1), ("2^63-1", I63 - 1), ("stream-length", total)]:
            extra.body_length = blen
            assert len(F.build(s)) == total
            out[f"{kind}-{name}"] = F.build(s)
    return out


# 8. flatbuffer damage
def metadata_of(stream: bytes, index: int):
    """(Reader over the index-th message's metadata, its position in the stream)"""
    at, size, _ = F.split_messages(stream)[0][index]
    return F.Reader(stream[at:at + size]), at


def patched(stream: bytes, pos: int, fmt: str, value) -> bytes:
    b = bytearray(stream)
    struct.pack_into("<" + fmt, b, pos, value)
    return bytes(b)


@functools.lru_cache(maxsize=None)
def damaged_flatbuffers() -> dict:
    out = {}
    good = F.build(F.describe(base_batch()))
    for index, which in ((0, "schema"), (1, "batch")):
        r, at = metadata_of(good, index)
        m = r.root()
        vt, size, _ = r.vtable(m)
        out[f"{which}-root-offset-outside"] = patched(good, at, "I", len(r.b) + 64)
        out[f"{which}-root-offset-huge"] = patched(good, at, "I", 0xFFFFFFF0)
        out[f"{which}-vtable-offset-below"] = patched(good, at + m, "i", m + 4096)
        out[f"{which}-vtable-offset-above"] = patched(good, at + m, "i", -(len(r.b) + 4096))
        out[f"{which}-vtable-offset-min"] = patched(good, at + m, "i", -2**31)
        out[f"{which}-vtable-size-2"] = patched(good, at + vt, "H", 2)
        out[f"{which}-vtable-size-3"] = patched(good, at + vt, "H", 3)
        out[f"{which}-field-offset-beyond-table"] = patched(good, at + vt + 4 + 2 * 2, "H", 0xFFF0)     # Message.header
        out[f"{which}-header-offset-outside"] = patched(good, at + r.field(m, 2), "I", 0x7FFFFFF0)
    r, at = metadata_of(good, 1)
    h = r.ref(r.root(), 2)
    for fid, name in ((1, "nodes"), (2, "buffers")):
        p, _ = r.vector(h, fid, 16)
        out[f"{name}-vector-length-2^32-1"] = patched(good, at + p - 4, "I", 0xFFFFFFFF)
        out[f"{name}-vector-length-2^28"] = patched(good, at + p - 4, "I", 1 << 28)
    r, at = metadata_of(good, 0)
    h = r.ref(r.root(), 2)
    p, _ = r.vector(h, 1, 4)
    out["fields-vector-length-2^32-1"] = patched(good, at + p - 4, "I", 0xFFFFFFFF)
    f0 = r.tables(h, 1)[0]
    out["name-string-beyond-buffer"] = patched(good, at + r.ref(f0, 0), "I", len(r.b))
    out["name-string-2^32-1"] = patched(good, at + r.ref(f0, 0), "I", 0xFFFFFFFF)
    return out


def mutated_streams(count: int = 500, seed: int = 20260):
    """`count` copies of a valid 11-column stream, each with one to four random byte or 32-bit overwrites inside its metadata"""
    from tests.test_ipc import sample_batch
    good = pyarrow_stream(sample_batch(50, seed=9))
    spans = [(at, size) for at, size, _ in F.split_messages(good)[0]]
    rng = np.random.default_rng(seed)
    for _ in range(count):
        b = bytearray(good)
        for _ in range(int(rng.integers(1, 5))):
            at, size = spans[int(rng.integers(0, len(spans)))]
            if rng.random() < 0.5:
                b[at + int(rng.integers(0, size))] = int(rng.integers(0, 256))
            else:
                value = int(rng.choice([0, 1, 0xFFFFFFFF, 0x7FFFFFFF, 0x80000000, int(rng.integers(0, 2**32)), int(rng.integers(0, 64))]))
                struct.pack_into("<I", b, at + int(rng.integers(0, size - 3)), value)
        yield bytes(b)


def run_sweep() -> None:
    """the child process of the mutation sweep: prints one line `sweep <checked> bad <list>`"""
    import chapterhouseqe_amd as chq
    bad, checked = [], 0
    for i, stream in enumerate(mutated_streams()):
        try:
            chq.ipc_describe(stream)
            code = 0
        except chq.ChqError as e:
            code = e.code
        checked += 1
        if code not in (0, 22, 30):
            bad.append((i, code))
    print(f"sweep {checked} bad {bad}")


def run_describe(path: str) -> None:
    """the child process of the skipped-message cases: exits with the status of ipc_describe on the file's bytes"""
    import chapterhouseqe_amd as chq
    with open(path, "rb") as f:
        stream = f.read()
    try:
        chq.ipc_describe(stream)
    except chq.ChqError as e:
        sys.exit(e.code)
    sys.exit(0)


# 9. malformed type tables: (tag, type fields, the fixed width a lenient reader would take it for)
TYPE_TABLES = {
    "int-24": (F.INT, [(0, "i", 24), (1, "?", True)]), "int-128": (F.INT, [(0, "i", 128), (1, "?", True)]),
    "float-precision-3": (F.FLOAT, [(0, "h", 3)]), "float-precision-7": (F.FLOAT, [(0, "h", 7)]),
    "date-unit-2": (F.DATE, [(0, "h", 2)]), "date-unit-5": (F.DATE, [(0, "h", 5)]),
    "time-second-64": (F.TIME, [(0, "h", 0), (1, "i", 64)]), "time-nanosecond-32": (F.TIME, [(0, "h", 3), (1, "i", 32)]),
    "time-unit-6": (F.TIME, [(0, "h", 6), (1, "i", 64)]), "time-unit-6-32": (F.TIME, [(0, "h", 6), (1, "i", 32)]),
    "timestamp-unit-4": (F.TIMESTAMP, [(0, "h", 4)]), "timestamp-unit-7": (F.TIMESTAMP, [(0, "h", 7)]),
    "duration-unit-4": (F.DURATION, [(0, "h", 4)]), "duration-unit-7": (F.DURATION, [(0, "h", 7)]),
    "decimal128-precision-0": (F.DECIMAL, [(0, "i", 0), (1, "i", 0), (2, "i", 128)]),
    "decimal128-precision-39": (F.DECIMAL, [(0, "i", 39), (1, "i", 0), (2, "i", 128)]),
    "fsb-minus-4": (F.FSB, [(0, "i", -4)]), "fsb-0": (F.FSB, [(0, "i", 0)]),
}


@functools.lru_cache(maxsize=None)
def type_table_cases() -> dict:
    """four rows in a 64-byte values buffer: wide enough for whichever width a lenient reader would pick"""
    out = {}
    for name, (tag, type_fields) in TYPE_TABLES.items():
        s = stream_of(pa.schema([pa.field("c", pa.int64())]), 4, [(4, 0)], [b"", bytes(range(64))])
        s.fields[0].type_tag, s.fields[0].type_fields = tag, type_fields
        out[name] = F.build(s)
    return out


# 10. Utf8 offsets with exactly one bad entry
@functools.lru_cache(maxsize=2)
def offsets_stream(n: int):
    """(stream of one Utf8 column of n two-byte strings, position of its offsets buffer in the stream, the batch)"""
    offs = np.arange(n + 1, dtype=np.int32) * 2
    data = np.resize(np.frombuffer(b"abcdefghijklmnopqrstuvwxyz", np.uint8), 2 * n)
    arr = pa.Array.from_buffers(pa.utf8(), n, [None, pa.py_buffer(offs.tobytes()), pa.py_buffer(data.tobytes())])
    rec = pa.RecordBatch.from_arrays([arr], names=["s"])
    stream = pyarrow_stream(rec)
    s = F.describe(stream)
    body_at = F.split_messages(stream)[0][1][2]
    assert s.batch.buffers[1][1] == 4 * (n + 1) and s.batch.buffers[2][1] == 2 * n
    return stream, body_at + s.batch.buffers[1][0], rec


def bad_offsets(n: int, row: int, kind: str) -> bytes:
    stream, at, _ = offsets_stream(n)
    if kind == "negative":          # the row starts below zero
        return patched(stream, at + 4 * row, "i", -1)
    if kind == "decreasing":        # the row ends before it starts
        return patched(stream, at + 4 * (row + 1), "i", 2 * row - 1) if row else patched(stream, at, "i", 3)
    assert kind == "beyond"         # the row ends behind the data
    return patched(stream, at + 4 * (row + 1), "i", 2 * n + 5)
