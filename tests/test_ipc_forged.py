"""`chq_record_from_ipc` / `chq_ipc_describe` (csrc/ipc.cpp) on forged Arrow IPC streams (tests/ipc_forge.py builds them,
tests/ipc_forged_cases.py lists them).  The decoder takes bytes another process wrote, copies the body into HBM and hands out
columns that kernels follow without further checks, so:

  A  legal streams no pyarrow writer emits are read bit-exact like pyarrow reads the same bytes
  B  legal streams outside the build's scope answer CHQ_ERR_NOT_SUPPORTED (30) and name the feature
  C  illegal streams answer CHQ_ERR_ARROW_INVALID_ARGUMENT (22): never a crash, a hang or a batch; the context stays usable
  D  the four small IPC kernels beyond one grid (4096 x 256 threads)
Whatever the metadata alone gives away is also checked without a GPU through `ipc_describe`."""
import os
import subprocess
import sys

import numpy as np
import pyarrow as pa
import pytest

import chapterhouseqe_amd as chq

from . import ipc_forge as F
from . import ipc_forged_cases as C
from .helpers import batches_identical, explain_diff

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, NOT_SUPPORTED = 22, 30


def describe_code(stream: bytes):
    try:
        return 0, chq.ipc_describe(stream)
    except chq.ChqError as e:
        return e.code, str(e)


# ------------------------------------------------------------------------------------------------------------ CPU tier
@pytest.mark.parametrize("name", sorted(C.legal_cases()))
def test_describe_reads_the_legal_forged_streams(name):
    stream, declared = C.legal_cases()[name]
    code, text = describe_code(stream)
    assert code == 0, text
    lines = text.splitlines()
    assert int(lines[0].split()[1]) == declared.num_rows
    fields = [l.split() for l in lines if l.startswith("field ")]
    assert [f[1] for f in fields] == declared.schema.names
    assert [f[3] for f in fields] == [f"nullable={int(fl.nullable)}" for fl in declared.schema]


def test_describe_reads_every_type_of_the_coverage_list():
    """FixedSizeBinary(3) among them: a width the decode places although no kernel moves it"""
    rec = C.coverage_batch(7, seed=7)
    code, text = describe_code(C.pyarrow_stream(rec))
    assert code == 0, text
    assert [l.split()[1] for l in text.splitlines() if l.startswith("field ")] == rec.schema.names


@pytest.mark.parametrize("name", sorted(C.out_of_scope_cases()))
def test_describe_names_what_is_out_of_scope(name):
    stream, word = C.out_of_scope_cases()[name]
    code, text = describe_code(stream)
    assert code == NOT_SUPPORTED and word in text, (code, text)


@pytest.mark.parametrize("name", sorted(C.illegal_cases()))
def test_describe_refuses_illegal_metadata(name):
    code, text = describe_code(C.illegal_cases()[name])
    assert code == INVALID, (code, text)


@pytest.mark.parametrize("name", sorted(C.damaged_flatbuffers()))
def test_describe_refuses_damaged_flatbuffers(name):
    code, text = describe_code(C.damaged_flatbuffers()[name])
    assert code == INVALID, (code, text)


@pytest.mark.parametrize("name", sorted(C.type_table_cases()))
def test_describe_refuses_malformed_type_tables(name):
    """each is refused, none is accepted under another type's width"""
    code, text = describe_code(C.type_table_cases()[name])
    assert code in (INVALID, NOT_SUPPORTED), (code, text)


def child(code: str, timeout: float):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)


@pytest.mark.parametrize("name", sorted(C.skipped_message_cases()))
def test_a_skipped_message_cannot_lead_the_cursor_astray(name, tmp_path):
    """in a fresh interpreter under a 20 s limit: the parent commit never returns from `back-to-itself`"""
    path = tmp_path / "stream.bin"
    path.write_bytes(C.skipped_message_cases()[name])
    done = child(f"from tests.ipc_forged_cases import run_describe; run_describe({str(path)!r})", 20)
    assert done.returncode == INVALID, (done.returncode, done.stderr[-500:])


def test_mutation_sweep_ends_normally():
    """500 streams with one to four random overwrites inside the metadata, one child process: every call answers 0, 22 or 30"""
    done = child("from tests.ipc_forged_cases import run_sweep; run_sweep()", 120)
    assert done.returncode == 0, (done.returncode, done.stderr[-500:])
    assert done.stdout.strip().splitlines()[-1] == "sweep 500 bad []", done.stdout[-500:]


# ------------------------------------------------------------------------------------------------------------ GPU tier
@pytest.fixture(scope="module")
def ctx():
    c = chq.Context(0)
    yield c
    c.close()


GOOD = C.base_batch(300, seed=77)
GOOD_STREAM = C.pyarrow_stream(GOOD)


def still_usable(c, device_result):
    got = chq.record_from_ipc(GOOD_STREAM, ctx=c, device_result=device_result)
    got = got.to_host() if device_result else got
    assert batches_identical(got, GOOD), explain_diff(got, GOOD)


def refused(c, stream, codes=(INVALID,), word=None, **how):
    """both result kinds refuse, nothing comes back, and the same context decodes a good stream afterwards"""
    for device_result in (True, False):
        with pytest.raises(chq.ChqError) as ei:
            chq.record_from_ipc(stream, ctx=c, device_result=device_result, **how)
        assert ei.value.code in codes, (ei.value.code, str(ei.value))
        assert word is None or word in str(ei.value), str(ei.value)
        still_usable(c, device_result)


def decoded(c, stream, device_result, **how):
    got = chq.record_from_ipc(stream, ctx=c, device_result=device_result, **how)
    return got.to_host() if device_result else got


def on_device(body: bytes):
    import torch
    return torch.frombuffer(bytearray(body), dtype=torch.uint8).to("cuda:0")


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(C.legal_cases()))
def test_legal_forged_streams_read_like_pyarrow_reads_them(ctx, name):
    stream, _ = C.legal_cases()[name]
    want = F.read_back(stream)
    for device_result in (True, False):
        got = decoded(ctx, stream, device_result)
        assert batches_identical(got, want), (device_result, explain_diff(got, want))
    header, body = F.header_and_body(F.describe(stream))
    if body:                                                       # the exchange's shape: metadata on the host, the body in HBM
        t = on_device(body)
        for device_result in (True, False):
            got = decoded(ctx, header, device_result, body_address=t.data_ptr(), body_len=len(body), body_on_device=True)
            assert batches_identical(got, want), (device_result, explain_diff(got, want))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 7, 63, 65])
def test_kernels_do_not_read_padding_bits(ctx, n):
    """junk behind the last row of validity and Boolean buffers: the filter kernels over the decoded device batch"""
    from chapterhouseqe_amd.sqlparse import parse_expr
    from oracle import oracle as O
    stream, rec = C.legal_cases()[f"padding-junk-{n}"]
    dev = chq.record_from_ipc(stream, ctx=ctx, device_result=True)
    al = [[] for _ in range(rec.num_columns)]
    for sql in ("flag", "flag = false", "flag = true or x > 600", "x > 0", "x <= 0 or x > 500", "x % 2 = 0 and f > 0.25"):
        e = parse_expr(sql)
        got = chq.filter_record(dev, al, e, ctx=ctx).to_host()
        want = O.filter_record(rec, al, e)
        assert batches_identical(got, want), (sql, explain_diff(got, want))


COVERAGE_N = [0, 1, 65, 4097]


@pytest.mark.gpu
@pytest.mark.parametrize("n", COVERAGE_N)
def test_type_coverage_the_gpu_reads_what_pyarrow_writes(ctx, n):
    for rec in (C.coverage_batch(n, seed=n), C.coverage_batch(n + 3, seed=n).slice(3)):
        stream = C.pyarrow_stream(rec)
        for device_result in (True, False):
            got = decoded(ctx, stream, device_result)
            assert got.schema.equals(rec.schema, check_metadata=False) and batches_identical(got, rec), explain_diff(got, rec)


@pytest.mark.gpu
@pytest.mark.parametrize("n", COVERAGE_N)
def test_type_coverage_pyarrow_reads_what_the_gpu_writes(ctx, n):
    for rec in (C.coverage_batch(n, seed=n), C.coverage_batch(n + 3, seed=n).slice(3)):
        for src in (rec, chq.DeviceRecordBatch.from_host(rec, ctx)):
            got = F.read_back(chq.record_to_ipc(src, ctx=ctx).to_bytes())
            assert got.schema.types == rec.schema.types and got.schema.equals(rec.schema, check_metadata=False)
            assert batches_identical(got, rec), explain_diff(got, rec)


@pytest.mark.gpu
def test_fixed_size_binary_3_round_trips(ctx):
    """a width no kernel moves (they copy values of 1, 2, 4, 8 and 16 bytes): the IPC paths and the staging copies place its
    bytes, and an operator that would launch a kernel on the column still answers 30 instead of reading it as a wider type"""
    from chapterhouseqe_amd.sqlparse import parse_expr
    rng = np.random.default_rng(3)
    rec = pa.RecordBatch.from_arrays([C.random_array(rng, pa.binary(3), 65, True), pa.array(np.arange(65, dtype=np.int32))], names=["w3", "x"])
    stream = C.pyarrow_stream(rec)
    for device_result in (True, False):
        assert batches_identical(decoded(ctx, stream, device_result), rec)
    dev = chq.record_from_ipc(stream, ctx=ctx, device_result=True)
    for src in (rec, dev):
        assert batches_identical(F.read_back(chq.record_to_ipc(src, ctx=ctx).to_bytes()), rec)
        with pytest.raises(chq.ChqError) as ei:
            chq.filter_record(src, [[], []], parse_expr("x > 3"), ctx=ctx)
        assert ei.value.code == NOT_SUPPORTED and "w:3" in str(ei.value), str(ei.value)


@pytest.mark.gpu
def test_out_of_scope_streams_are_named(ctx):
    for name, (stream, word) in sorted(C.out_of_scope_cases().items()):
        refused(ctx, stream, codes=(NOT_SUPPORTED,), word=word)


@pytest.mark.gpu
def test_illegal_metadata_is_refused_before_the_body_moves(ctx):
    cases = {**C.illegal_cases(), **C.damaged_flatbuffers()}
    for name, stream in sorted(cases.items()):
        refused(ctx, stream)
    for name, stream in sorted(C.type_table_cases().items()):
        refused(ctx, stream, codes=(INVALID, NOT_SUPPORTED))


@pytest.mark.gpu
def test_a_null_count_that_contradicts_the_bitmap(ctx):
    """the node says 5 where 9 bits are clear (and 9 where 5 are): refused, or exported with the TRUE count -- never the forged one"""
    n = 65
    for claimed, clear in ((5, 9), (9, 5), (1, 0), (64, 65)):
        valid = np.ones(n, bool)
        valid[np.arange(clear) * 7 % n] = False
        assert int((~valid).sum()) == clear
        bitmap = C.junk_padding(np.packbits(valid, bitorder="little").tobytes() + bytes(7), n)
        s = C.stream_of(pa.schema([pa.field("x", pa.int32())]), n, [(n, claimed)], [bitmap, np.arange(n, dtype=np.int32).tobytes()], lead=8)
        stream = F.build(s)
        for device_result in (True, False):
            try:
                got = decoded(ctx, stream, device_result)
            except chq.ChqError as e:
                assert e.code == INVALID, (e.code, str(e))
            else:
                assert got.column(0).null_count == clear and int((~np.asarray(got.column(0).is_valid())).sum()) == clear
            still_usable(ctx, device_result)


@pytest.mark.gpu
def test_a_separate_body_shorter_than_the_metadata_says(ctx):
    header, body = F.header_and_body(F.describe(C.base_batch()))
    t = on_device(body)
    host = np.frombuffer(body, np.uint8).copy()
    for short in (len(body) - 1, len(body) - 64, 8):
        refused(ctx, header, body_address=t.data_ptr(), body_len=short, body_on_device=True)
        refused(ctx, header, body_address=host.ctypes.data, body_len=short, body_on_device=False)
    refused(ctx, header)                                            # no body at all
    want = C.base_batch()
    got = decoded(ctx, header, True, body_address=host.ctypes.data, body_len=len(body), body_on_device=False)
    assert batches_identical(got, want)


@pytest.mark.gpu
def test_two_batches_are_refused_like_the_reference_does(ctx):
    """ExchangeRequestsError::ReceivedMultipleRecordBatches: inline bodies, and two batch messages in front of a separate body"""
    refused(ctx, C.illegal_cases()["two-batches"], word="more than one record batch")
    header, body = C.two_batch_header_and_body()
    t = on_device(body)
    refused(ctx, header, word="more than one record batch", body_address=t.data_ptr(), body_len=len(body), body_on_device=True)


SMALL_N, BIG_N = 300, 2**20 + 257          # BIG_N: row 2^20 + 3 is seen by the second grid-stride trip of the check alone
BAD_ROWS = [(SMALL_N, 0), (SMALL_N, SMALL_N - 1), (SMALL_N, 255), (SMALL_N, 256), (BIG_N, 2**20 + 3)]


@pytest.mark.gpu
@pytest.mark.parametrize("n,row", BAD_ROWS)
def test_one_bad_utf8_offset_is_found(ctx, n, row):
    stream, _, rec = C.offsets_stream(n)
    for device_result in (True, False):                            # the same column without the defect
        got = decoded(ctx, stream, device_result)
        assert got.num_rows == n and got.column(0).equals(rec.column(0))
    for kind in ("negative", "decreasing", "beyond"):
        bad = C.bad_offsets(n, row, kind)
        assert int((np.frombuffer(bad, np.int32) != np.frombuffer(stream, np.int32)).sum()) == 1      # exactly one bad offset
        refused(ctx, bad, word="offsets")


# ---- D: beyond one grid of the IPC kernels ---------------------------------------------------------------------------------
@pytest.mark.gpu
def test_utf8_offsets_beyond_one_grid(ctx):
    """2^20 + 300 short strings sliced at row 3: rebase_offsets_kernel on the way out, validate_offsets_kernel on the way in"""
    n = 2**20 + 303
    rng = np.random.default_rng(5)
    lengths = rng.integers(0, 4, n)
    offs = np.zeros(n + 1, np.int32)
    np.cumsum(lengths, out=offs[1:])
    data = rng.integers(ord("a"), ord("z") + 1, int(offs[-1])).astype(np.uint8)
    full = pa.RecordBatch.from_arrays([pa.Array.from_buffers(pa.utf8(), n, [None, pa.py_buffer(offs.tobytes()), pa.py_buffer(data.tobytes())])], names=["s"])
    rec = full.slice(3)
    assert rec.num_rows == 2**20 + 300
    for src in (rec, chq.DeviceRecordBatch.from_host(full, ctx).slice(3, n - 3)):
        got = F.read_back(chq.record_to_ipc(src, ctx=ctx).to_bytes())
        assert got.column(0).equals(rec.column(0))
        assert np.frombuffer(got.column(0).buffers()[1], np.int32, n - 2)[0] == 0              # rebased
    stream = C.pyarrow_stream(rec)
    for device_result in (True, False):
        assert decoded(ctx, stream, device_result).column(0).equals(rec.column(0))


@pytest.mark.gpu
def test_bitmaps_beyond_one_grid(ctx):
    """a nullable Boolean column of 2^25 + 77 rows as a device view at offset 3 with an unknown null count:
    bit_shift_copy_kernel for both bitmaps and count_bits_kernel past their first grid-stride trip"""
    n, off = 2**25 + 80, 3
    rng = np.random.default_rng(8)
    values, valid = rng.random(n) < 0.5, rng.random(n) < 0.9
    rec = pa.RecordBatch.from_arrays([pa.array(values, mask=~valid)], names=["flag"])
    view = chq.DeviceRecordBatch.from_host(rec, ctx).slice(off, n - off)
    col = view.describe_columns()[0]
    assert view.num_rows == 2**25 + 77 and col["offset"] == off and col["validity"] and col["null_count"] == -1
    got = F.read_back(chq.record_to_ipc(view, ctx=ctx).to_bytes()).column(0)
    rows = n - off
    assert len(got) == rows and got.offset == 0
    got_valid = np.unpackbits(np.frombuffer(got.buffers()[0], np.uint8), bitorder="little")[:rows].astype(bool)
    got_values = np.unpackbits(np.frombuffer(got.buffers()[1], np.uint8), bitorder="little")[:rows].astype(bool)
    assert np.array_equal(got_valid, valid[off:])
    assert np.array_equal(got_values & got_valid, values[off:] & valid[off:])
    assert got.null_count == int((~valid[off:]).sum())
