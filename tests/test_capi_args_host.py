"""The C ABI's argument contract that needs no GPU: a null context is CHQ_ERR_INVALID_HANDLE before the caller's output
structs are touched, the entries that answer with text in a caller's buffer, and the expression-handle constructors under the
host sanitizers.  The calls go to the library raw (`_lib.lib()`), the way a foreign binding makes them.  Every call here is
decided by an explicit check of the library; tests/test_gpu_capi_args.py pins the checks behind a live context."""
import ctypes as C
import io
import os
import re
import shutil
import subprocess

import pyarrow as pa
import pyarrow.parquet as pq
import pytest

from chapterhouseqe_amd import _lib
from chapterhouseqe_amd.record_utils import _export_host, _expr_to_c
from chapterhouseqe_amd.sqlparse import parse_expr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID_ARGUMENT, INVALID_HANDLE = 0, 22, 31
CPU = _lib.ARROW_DEVICE_CPU
PDA = C.POINTER(_lib.ArrowDeviceArray)


def poisoned(ctype, n=1):
    """n structs of `ctype`, every byte 0xAB"""
    arr = (ctype * n)()
    C.memset(arr, 0xAB, C.sizeof(arr))
    return arr


def untouched(arr) -> bool:
    return bytes(arr) == b"\xab" * C.sizeof(arr)


def vp(arr):
    return C.cast(arr, C.c_void_p)


def parquet_bytes() -> bytes:
    sink = io.BytesIO()
    pq.write_table(pa.table({"id": pa.array([1, 2, 3], pa.int32())}), sink)
    return sink.getvalue()


class Args:
    """valid-looking arguments of every entry: one host batch, one expression, one of every key / item struct"""

    def __init__(self):
        L = _lib.lib()
        rec = pa.RecordBatch.from_arrays([pa.array([3, 1, 2], pa.int32()), pa.array(["a", "b", "c"]), pa.array([1.0, 2.0, 3.0], pa.float32())],
                                         names=["id", "s", "v"])
        self.cb = _export_host(rec)
        self.rec, self.schema = C.pointer(self.cb.array), C.pointer(self.cb.schema)
        self.recs = (PDA * 1)(self.rec)
        self.expr = _expr_to_c(parse_expr("id > 1"))
        self.col = _expr_to_c(parse_expr("id"))
        self.exprs = (C.c_void_p * 1)(self.col)
        self.sort_keys = (_lib.SortKey * 1)(_lib.SortKey(self.col, 0, 0))
        self.agg_items = (_lib.AggItem * 1)(_lib.AggItem(1, 0, None, b"n"))
        self.win_items = (_lib.WindowItem * 1)(_lib.WindowItem(0, 0, 0, None, b"rn"))
        self.join_keys = (_lib.JoinKey * 1)(_lib.JoinKey(self.col, self.col))
        self.select = (_lib.SelectItem * 1)(_lib.SelectItem(0, None, None))
        self.descs = (_lib.ColumnDesc * 1)()
        self.file = parquet_bytes()
        self.pq = C.c_void_p()
        assert L.chq_parquet_open(self.file, len(self.file), C.byref(self.pq), None, 0) == OK and self.pq

    def close(self):
        L = _lib.lib()
        L.chq_parquet_close(self.pq)
        L.chq_expr_free(self.expr)
        L.chq_expr_free(self.col)
        self.cb.release()


@pytest.fixture(scope="module")
def args():
    a = Args()
    yield a
    a.close()


# entry -> call(L, a, ctx, pq, out, out_schema) -> status.  `out` / `out_schema` are the poisoned outputs: one
# ArrowDeviceArray + ArrowSchema, or (OUTPUTS) the entry's own output struct.
RECORD_CALLS = {
    "chq_filter_record": lambda L, a, ctx, pq, o, s: L.chq_filter_record(ctx, a.rec, a.schema, None, a.expr, CPU, o, s),
    "chq_filter_records": lambda L, a, ctx, pq, o, s: L.chq_filter_records(ctx, 1, a.recs, a.schema, None, a.expr, CPU, o, s),
    "chq_filter_records_coalesced": lambda L, a, ctx, pq, o, s: L.chq_filter_records_coalesced(ctx, 1, a.recs, a.schema, None, a.expr, CPU, o, s, None),
    "chq_project_record": lambda L, a, ctx, pq, o, s: L.chq_project_record(ctx, a.select, 1, a.rec, a.schema, None, CPU, o, s),
    "chq_compute_value": lambda L, a, ctx, pq, o, s: L.chq_compute_value(ctx, a.rec, a.schema, None, a.expr, CPU, o, s, None),
    "chq_filter_project_record": lambda L, a, ctx, pq, o, s: L.chq_filter_project_record(ctx, a.expr, a.select, 1, a.rec, a.schema, None, CPU, o, s),
    "chq_record_to_device": lambda L, a, ctx, pq, o, s: L.chq_record_to_device(ctx, a.rec, a.schema, o, s),
    "chq_record_to_host": lambda L, a, ctx, pq, o, s: L.chq_record_to_host(ctx, a.rec, a.schema, o, s),
    "chq_wrap_columns": lambda L, a, ctx, pq, o, s: L.chq_wrap_columns(ctx, a.descs, 0, 0, CPU, o, s),
    "chq_record_copy_to_peer": lambda L, a, ctx, pq, o, s: L.chq_record_copy_to_peer(ctx, ctx, a.rec, a.schema, o, s),
    "chq_record_from_ipc": lambda L, a, ctx, pq, o, s: L.chq_record_from_ipc(ctx, a.file, len(a.file), None, 0, CPU, CPU, o, s),
    "chq_parquet_read_row_group": lambda L, a, ctx, pq, o, s: L.chq_parquet_read_row_group(ctx, pq, 0, CPU, o, s),
    "chq_parquet_read_row_groups": lambda L, a, ctx, pq, o, s: L.chq_parquet_read_row_groups(ctx, pq, 0, 1, CPU, vp(o), vp(s)),
    "chq_parquet_read_columns": lambda L, a, ctx, pq, o, s: L.chq_parquet_read_columns(ctx, pq, 0, 1, None, -1, CPU, vp(o), vp(s)),
    "chq_sort_record": lambda L, a, ctx, pq, o, s: L.chq_sort_record(ctx, a.rec, a.schema, None, a.sort_keys, 1, -1, CPU, o, s),
    "chq_sort_records": lambda L, a, ctx, pq, o, s: L.chq_sort_records(ctx, 1, a.recs, a.schema, None, a.sort_keys, 1, -1, CPU, o, s),
    "chq_aggregate_record": lambda L, a, ctx, pq, o, s: L.chq_aggregate_record(ctx, a.rec, a.schema, None, a.exprs, 1, a.agg_items, 1, CPU, o, s),
    "chq_aggregate_records": lambda L, a, ctx, pq, o, s: L.chq_aggregate_records(ctx, 1, a.recs, a.schema, None, a.exprs, 1, a.agg_items, 1, CPU, o, s),
    "chq_window_record": lambda L, a, ctx, pq, o, s: L.chq_window_record(ctx, a.rec, a.schema, None, a.exprs, 1, a.sort_keys, 1, a.win_items, 1, CPU, o, s),
    "chq_window_records": lambda L, a, ctx, pq, o, s: L.chq_window_records(ctx, 1, a.recs, a.schema, None, a.exprs, 1, a.sort_keys, 1, a.win_items, 1, CPU, o, s),
    "chq_join_records": lambda L, a, ctx, pq, o, s: L.chq_join_records(ctx, 1, a.recs, a.schema, None, 1, a.recs, a.schema, None, a.join_keys, 1, CPU, o, s),
    "chq_join_records_kind": lambda L, a, ctx, pq, o, s: L.chq_join_records_kind(ctx, 1, a.recs, a.schema, None, 1, a.recs, a.schema, None, a.join_keys, 1, 1, CPU, o, s),
    "chq_partition_records": lambda L, a, ctx, pq, o, s: L.chq_partition_records(ctx, 1, a.recs, a.schema, None, a.exprs, 1, 1, CPU, o, s),
}
OUTPUTS = {   # the entries whose output is a struct of its own
    "chq_record_to_ipc": (_lib.IpcMessage, lambda L, a, ctx, o: L.chq_record_to_ipc(ctx, a.rec, a.schema, CPU, o)),
    "chq_record_to_parquet": (_lib.ParquetImage, lambda L, a, ctx, o: L.chq_record_to_parquet(ctx, a.rec, a.schema, o)),
    "chq_records_to_parquet": (_lib.ParquetImage, lambda L, a, ctx, o: L.chq_records_to_parquet(ctx, 1, a.recs, a.schema, o)),
}
CTX_ACCESSORS = {"chq_ctx_create", "chq_ctx_destroy", "chq_ctx_last_error", "chq_ctx_stream", "chq_ctx_set_option", "chq_ctx_last_stats"}
NO_CONTEXT = {"chq_abi_version", "chq_status_name", "chq_plan_describe", "chq_ipc_describe", "chq_parquet_open", "chq_parquet_open_reader",
              "chq_parquet_num_columns", "chq_parquet_column_name", "chq_parquet_close", "chq_parquet_num_row_groups",
              "chq_parquet_row_group_num_rows", "chq_parquet_describe"}
TAKES_PARQUET = ("chq_parquet_read_row_group", "chq_parquet_read_row_groups", "chq_parquet_read_columns")


def test_every_exported_entry_is_accounted_for():
    """a new entry must be given a place here: with a context (and a null-context case below) or without"""
    names = set(_lib.EXPORTED_SYMBOLS)
    exprs = {n for n in names if n.startswith("chq_expr_")}
    covered = set(RECORD_CALLS) | set(OUTPUTS) | CTX_ACCESSORS | NO_CONTEXT | exprs
    assert names == covered, (sorted(names - covered), sorted(covered - names))


@pytest.mark.parametrize("name", sorted(RECORD_CALLS))
def test_null_context_leaves_the_outputs_untouched(args, name):
    L = _lib.lib()
    out, out_schema = poisoned(_lib.ArrowDeviceArray), poisoned(_lib.ArrowSchema)
    assert RECORD_CALLS[name](L, args, None, args.pq, out, out_schema) == INVALID_HANDLE
    assert untouched(out) and untouched(out_schema)
    if name in TAKES_PARQUET:   # no file either
        assert RECORD_CALLS[name](L, args, None, None, out, out_schema) == INVALID_HANDLE
        assert untouched(out) and untouched(out_schema)


@pytest.mark.parametrize("name", sorted(OUTPUTS))
def test_null_context_leaves_the_output_struct_untouched(args, name):
    ctype, call = OUTPUTS[name]
    out = poisoned(ctype)
    assert call(_lib.lib(), args, None, out) == INVALID_HANDLE
    assert untouched(out)


def test_context_accessors_take_a_null_context():
    L = _lib.lib()
    assert L.chq_ctx_last_error(None) == b"null context"
    assert L.chq_ctx_stream(None) is None
    stats = poisoned(_lib.CallStats)
    L.chq_ctx_last_stats(None, stats)
    assert untouched(stats)
    assert L.chq_ctx_set_option(None, b"tile_kind", 0) == INVALID_HANDLE
    assert L.chq_ctx_create(0, None, None) == INVALID_HANDLE
    L.chq_ctx_destroy(None)


# ---- text in the caller's buffer ---------------------------------------------------------------------------------------------
def text_call(call, text: bytes, fits_status: int, short_status: int):
    """`call(buf, buf_len)` answers `text`: what the caller's buffer holds for buf_len 0, 1, len(text) and len(text) + 1"""
    for buf_len in (0, 1, len(text), len(text) + 1):
        buf = C.create_string_buffer(b"\xab" * (len(text) + 8), len(text) + 8)
        st = call(buf, buf_len)
        assert st == (fits_status if buf_len > len(text) else short_status), buf_len
        kept = text[:max(0, buf_len - 1)]
        expect = (kept + b"\0" if buf_len else b"") + b"\xab" * (len(text) + 8)
        assert buf.raw == expect[:len(text) + 8], buf_len
    assert call(None, len(text) + 1) == fits_status


def test_plan_describe_without_an_expression(args):
    L = _lib.lib()
    text_call(lambda buf, n: L.chq_plan_describe(args.schema, None, None, 3, 0, buf, n), b"null expression", INVALID_HANDLE, INVALID_HANDLE)


def test_plan_describe_text_is_cut_to_the_buffer(args):
    L = _lib.lib()
    buf = C.create_string_buffer(4096)
    assert L.chq_plan_describe(args.schema, None, args.expr, 3, 0, buf, 4096) == OK
    text = buf.value
    assert len(text) > 8
    text_call(lambda b, n: L.chq_plan_describe(args.schema, None, args.expr, 3, 0, b, n), text, OK, OK)


def test_ipc_describe_without_a_stream():
    L = _lib.lib()
    text_call(lambda buf, n: L.chq_ipc_describe(None, 64, buf, n), b"empty Arrow IPC stream", INVALID_ARGUMENT, INVALID_ARGUMENT)


def test_parquet_open_without_a_file_or_a_handle(args):
    L = _lib.lib()
    h = C.c_void_p(0xABAB)
    text_call(lambda buf, n: L.chq_parquet_open(None, 64, C.byref(h), buf, n), b"parquet: file shorter than the magic numbers",
              INVALID_ARGUMENT, INVALID_ARGUMENT)
    assert not h   # the handle is cleared first
    buf = C.create_string_buffer(b"\xab" * 16, 16)
    assert L.chq_parquet_open(args.file, len(args.file), None, buf, 16) == INVALID_ARGUMENT
    assert buf.raw == b"\xab" * 16
    # success leaves an empty message
    assert L.chq_parquet_open(args.file, len(args.file), C.byref(h), buf, 16) == OK and h
    assert buf.raw == b"\0" + b"\xab" * 15
    L.chq_parquet_close(h)


def test_parquet_open_reader_without_a_reader_or_a_handle(args):
    L = _lib.lib()
    h = C.c_void_p(0xABAB)
    no_reader = _lib.READ_RANGE_FN()
    text_call(lambda buf, n: L.chq_parquet_open_reader(len(args.file), no_reader, None, C.byref(h), buf, n), b"null range reader",
              INVALID_HANDLE, INVALID_HANDLE)
    assert not h
    buf = C.create_string_buffer(b"\xab" * 16, 16)
    assert L.chq_parquet_open_reader(len(args.file), no_reader, None, None, buf, 16) == INVALID_ARGUMENT
    assert buf.raw == b"\xab" * 16


def test_parquet_describe_reports_a_short_buffer(args):
    L = _lib.lib()
    assert L.chq_parquet_describe(None, C.create_string_buffer(16), 16) == INVALID_HANDLE
    buf = C.create_string_buffer(8192)
    assert L.chq_parquet_describe(args.pq, buf, 8192) == OK
    text = buf.value
    assert len(text) > 8
    text_call(lambda b, n: L.chq_parquet_describe(args.pq, b, n), text, OK, INVALID_ARGUMENT)   # (a null buffer of room enough is OK too)
    assert L.chq_parquet_describe(args.pq, None, 0) == INVALID_ARGUMENT


def test_parquet_accessors_take_a_null_handle():
    L = _lib.lib()
    assert L.chq_parquet_num_columns(None) == 0 and L.chq_parquet_num_row_groups(None) == 0
    assert L.chq_parquet_column_name(None, 0) is None and L.chq_parquet_row_group_num_rows(None, 0) == -1
    L.chq_parquet_close(None)


# ---- the expression-handle constructors alone, under the sanitizers ------------------------------------------------------------
def test_expression_constructors_under_host_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler on PATH")
    exe = str(tmp_path / "capi_expr_main")
    flags = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    src = os.path.join(ROOT, "tests", "capi_expr_main.cpp")
    build = subprocess.run([cxx, *flags, "-static-libasan", "-static-libubsan", src, "-o", exe], capture_output=True, text=True)
    if build.returncode != 0:
        build = subprocess.run([cxx, *flags, src, "-o", exe], capture_output=True, text=True)
    if build.returncode != 0 and re.search(r"asan|ubsan|sanitize", build.stderr, re.I):
        pytest.skip("the compiler has no sanitizer runtime: " + build.stderr.strip().splitlines()[-1])
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    if run.returncode != 0 and "runtime does not come first" in run.stderr:
        pytest.skip("this environment preloads a library in front of the sanitizer runtime: " + run.stderr.strip().splitlines()[0])
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    m = re.fullmatch(r"(\d+) checks, 0 mismatches\n", run.stdout)
    assert m and int(m.group(1)) >= 80, run.stdout
