"""The Arrow IPC forge checked against pyarrow (CPU tier): what tests/ipc_forge.py builds from a description is read back by
`pa.ipc.open_stream` as the batch it describes, every knob does what it says, and every legal forged stream of
tests/ipc_forged_cases.py is read by pyarrow as the values the case declares."""
import struct

import pyarrow as pa
import pytest

from . import ipc_forge as F
from . import ipc_forged_cases as C
from .helpers import batches_identical, explain_diff
from .test_ipc import sample_batch


def same(got: pa.RecordBatch, want: pa.RecordBatch) -> bool:
    return got.schema.equals(want.schema, check_metadata=True) and batches_identical(got, want)


@pytest.mark.parametrize("n", [0, 1, 7, 1000])
@pytest.mark.parametrize("make", [sample_batch, C.coverage_batch], ids=["sample", "coverage"])
def test_build_of_describe_is_read_back_identically(make, n):
    rec = make(n, seed=n)
    s = F.describe(rec)
    assert s.version == F.V5 and not s.legacy_framing and s.eos and s.schema_at == 0 and s.batch.length == n
    assert len(s.batch.nodes) == rec.num_columns and [nc for _, nc in s.batch.nodes] == [c.null_count for c in rec.columns]
    got = F.read_back(F.build(s))
    assert same(got, rec), explain_diff(got, rec)
    again = F.describe(F.build(s))                      # the strict reader reads what the builder wrote
    assert again == s


def test_the_builder_lays_tables_out_as_asked():
    b = F.Builder()
    name = b.string("héllo")
    pairs = b.pair_vector([(1, 2), (2**63 - 8, -1)])
    t = b.table([(3, "q", -5), (0, "ref", name), (7, "B", 9), (1, "ref", pairs), (2, "ref", 0)], extra_slots=4)
    r = F.Reader(b.finish(t))
    root = r.root()
    assert r.slots(root) == 8 + 4                       # ids 0..7 and four empty entries behind them
    assert r.string(root, 0) == "héllo" and r.scalar(root, 3, "q", 0) == -5 and r.scalar(root, 7, "B", 0) == 9
    assert r.field(root, 2) is None and r.field(root, 11) is None and r.field(root, 40) is None
    p, n = r.vector(root, 1, 16)
    assert n == 2 and p % 8 == 0 and struct.unpack_from("<qqqq", r.b, p) == (1, 2, 2**63 - 8, -1)
    assert r.field(root, 3) % 8 == 0 and len(r.b) % 8 == 0
    assert r.field(root, 3) > r.field(root, 0) > r.field(root, 7)          # stored in the order given, the first highest


def test_the_strict_reader_refuses_damage():
    good = F.build(F.describe(C.base_batch()))
    F.describe(good)
    for name, stream in C.damaged_flatbuffers().items():
        with pytest.raises((F.ForgeError, UnicodeDecodeError)):
            F.describe(stream)


def framing(stream: bytes):
    frames, legacy, eos = F.split_messages(stream)
    return frames, legacy, eos


def test_knobs_do_what_they_say():
    rec = C.base_batch()
    plain = F.build(F.describe(rec))
    # legacy framing: no continuation marker anywhere, 4-byte end marker
    s = F.describe(rec)
    s.legacy_framing = True
    legacy = F.build(s)
    frames, is_legacy, eos = framing(legacy)
    assert is_legacy and eos and legacy[:4] != F.CONTINUATION and legacy.endswith(bytes(4)) and not legacy.endswith(F.CONTINUATION + bytes(4))
    assert all((body_at % 8) == 0 for _, _, body_at in frames) and frames[0][0] == 4
    assert same(F.read_back(legacy), rec)
    # V4 metadata: every message says so
    s = F.describe(rec)
    s.version = F.V4
    v4 = F.build(s)
    for at, size, _ in framing(v4)[0]:
        r = F.Reader(v4[at:at + size])
        assert r.scalar(r.root(), 0, "h", 0) == F.V4
    assert F.describe(v4).version == F.V4 and same(F.read_back(v4), rec)
    # shuffled body: other offsets, the same buffers
    order = [8, 3, 0, 6, 5, 1, 7, 2, 4]
    s = F.relaid(F.describe(rec), order=order, lead=8, gap=3, slack=13, trailing=21, filler=0xA5)
    base = F.describe(rec).batch
    placed = sorted((off, i) for i, (off, ln) in enumerate(s.batch.buffers))
    assert [i for _, i in placed] == order and s.batch.buffers[order[0]][0] == 8
    assert [b[:len(a)] for a, b in zip(F.buffer_bytes(base), F.buffer_bytes(s.batch))] == F.buffer_bytes(base)
    assert all(ln == len(a) + 13 for a, (_, ln) in zip(F.buffer_bytes(base), s.batch.buffers))
    assert s.batch.body[:8] == b"\xa5" * 8 and s.batch.body.endswith(b"\xa5" * 21) and len(s.batch.body) % 8 == 0
    assert same(F.read_back(F.build(s)), rec)
    # long vtables, padded metadata: longer metadata, the same reading
    s = F.describe(rec)
    s.extra_slots, s.batch.extra_slots, s.fields[0].extra_slots, s.meta_pad, s.tail_pad = 5, 6, 7, 16, 8
    long = F.build(s)
    at, size, _ = framing(long)[0][1]
    r = F.Reader(long[at:at + size])
    assert r.slots(r.root()) == 4 + 5 and r.slots(r.ref(r.root(), 2)) == 3 + 6 and long[at + size - 24:at + size] == bytes(24)
    assert framing(long)[0][1][1] > framing(plain)[0][1][1] and same(F.read_back(long), rec)
    # custom metadata on schema, field and message
    s = F.describe(rec)
    s.metadata, s.fields[2].metadata, s.batch.metadata = [("a", "b")], [("c", "d")], [("e", "f")]
    got = pa.ipc.open_stream(F.build(s))
    assert got.schema.metadata == {b"a": b"b"} and got.schema.field(2).metadata == {b"c": b"d"}
    assert got.read_next_batch_with_custom_metadata().custom_metadata == {b"e": b"f"}
    back = F.describe(F.build(s))
    assert back.metadata == s.metadata and back.fields[2].metadata == s.fields[2].metadata and back.batch.metadata == s.batch.metadata
    # no end marker; extra messages keep their place and body
    s = F.describe(rec)
    s.eos = False
    s.messages.append(F.Extra(F.TENSOR, 16, bytes(range(16))))
    back = F.describe(F.build(s))
    assert not back.eos and back.messages[1] == s.messages[1]


@pytest.mark.parametrize("name", sorted(C.legal_cases()))
def test_pyarrow_reads_the_legal_forged_streams_as_declared(name):
    stream, declared = C.legal_cases()[name]
    got = F.read_back(stream)
    assert same(got, declared), explain_diff(got, declared)


def test_the_forged_shapes_are_what_the_cases_say():
    """the properties the legal cases are about hold in the bytes pyarrow accepted"""
    s = F.describe(C.legal_cases()["validity-with-null-count-0"][0])
    assert s.batch.nodes[0][1] == 0 and any(b != 0xFF for b in F.buffer_bytes(s.batch)[0][:8])
    for n in (1, 7, 63, 65):
        s = F.describe(C.legal_cases()[f"padding-junk-{n}"][0])
        for i in (0, 2, 3, 4):
            last = F.buffer_bytes(s.batch)[i]
            assert all(last[k >> 3] >> (k & 7) & 1 for k in range(n, 8 * len(last))), (n, i)
    s = F.describe(C.legal_cases()["utf8-zero-rows-no-offsets"][0])
    assert s.batch.length == 0 and s.batch.buffers[1][1] == 0
    s = F.describe(C.legal_cases()["utf8-first-offset-nonzero"][0])
    assert struct.unpack_from("<i", F.buffer_bytes(s.batch)[1])[0] == 11
    s = F.describe(C.legal_cases()["metadata-everywhere"][0])
    assert s.batch.variadic == []
