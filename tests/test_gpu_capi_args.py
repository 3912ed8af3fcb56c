"""The C ABI's argument contract behind a live context: which status and which chq_ctx_last_error text a bad argument gets,
and which fault wins when several are present.  Each entry is pinned by peeling: the first call has every checkable argument
at fault at once and must report the entry's first check; that one argument is repaired and the call repeated, until it
succeeds.  The ordered (fault, status, message) lists below are the contract, read off the library's checks.

Every call here is decided by an explicit check of the library -- the test pins checks, it never finds out what an unchecked
pointer does.  Outputs are filled with 0xAB before every call: after a failed call they read as released (all zero), except
where a step says the entry leaves them untouched because it cannot know how many there are."""
import ctypes as C

import numpy as np
import pyarrow as pa
import pytest

import chapterhouseqe_amd as chq
from chapterhouseqe_amd import _lib
from chapterhouseqe_amd.record_utils import _export_host, _expr_to_c
from chapterhouseqe_amd.sqlparse import parse_expr

from .test_capi_args_host import INVALID_ARGUMENT as IA, INVALID_HANDLE as IH, OK, parquet_bytes, poisoned, untouched, vp

pytestmark = pytest.mark.gpu

NS = 30   # CHQ_ERR_NOT_SUPPORTED
CPU, ROCM = _lib.ARROW_DEVICE_CPU, _lib.ARROW_DEVICE_ROCM
PDA = C.POINTER(_lib.ArrowDeviceArray)
OUT_DEVICE = "out_device must be ARROW_DEVICE_CPU or ARROW_DEVICE_ROCM"
ONE_BATCH = "at least one record batch is needed"
MAX_PARTITIONS = 256   # kPartMaxPartitions


class Env:
    """one context, the 3-row batch host and device resident, and the handles the calls need"""

    def __init__(self):
        self.L = _lib.lib()
        self.ctx_obj = chq.Context(0)
        self.ctx = self.ctx_obj.handle
        rec = pa.RecordBatch.from_arrays([pa.array([3, 1, 2], pa.int32()), pa.array(["a", "b", "c"]), pa.array([1.0, 2.0, 3.0], pa.float32())],
                                         names=["id", "s", "v"])
        self.host = _export_host(rec)
        self.dev_obj = chq.DeviceRecordBatch.from_host(rec, self.ctx_obj)
        self.dev = self.dev_obj._cb
        self.pred = _expr_to_c(parse_expr("id > 1"))
        self.id = _expr_to_c(parse_expr("id"))
        self.v = _expr_to_c(parse_expr("v"))
        self.stream = chq.record_to_ipc(rec, ctx=self.ctx_obj).to_bytes()
        self.file = parquet_bytes()
        self.pq = C.c_void_p()
        assert self.L.chq_parquet_open(self.file, len(self.file), C.byref(self.pq), None, 0) == OK

    def error(self) -> str:
        return self.L.chq_ctx_last_error(self.ctx).decode()

    def close(self):
        self.L.chq_parquet_close(self.pq)
        for h in (self.pred, self.id, self.v):
            self.L.chq_expr_free(h)
        self.dev_obj.release()
        self.host.release()
        self.ctx_obj.close()


@pytest.fixture(scope="module")
def env():
    e = Env()
    yield e
    e.close()


def release(struct):
    if struct.release:
        C.CFUNCTYPE(None, C.c_void_p)(struct.release)(C.addressof(struct))


def rec_args(cb, v):
    """(rec, schema) of a single-record call"""
    return (C.pointer(cb.array) if v["rec"] else None, C.pointer(cb.schema) if v["schema"] else None)


def recs_arg(cb, v, given="recs", first="rec0"):
    """the record array of a group call: absent, or one element that may be null"""
    if not v[given]:
        return None
    return (PDA * 1)(C.pointer(cb.array)) if v[first] else (PDA * 1)()


def sort_keys_arg(v, given="keys", column="key0"):
    return (_lib.SortKey * 1)(_lib.SortKey(v[column], 0, 0)) if v[given] else None


def exprs_arg(v, given="keys", first="key0"):
    return (C.c_void_p * 1)(v[first]) if v[given] else None


# A spec: `good` (every argument valid), `steps` -- (argument, its faulty value, status, last_error, output structs cleared by
# the failed call) in the order the entry checks them -- and `call(env, v, o, s)`, which makes the C call from the plain values in `v`
# and the output arrays (None where v["out"] / v["out_schema"] is false).
ZEROED, UNTOUCHED = 1, 0   # how many of the output structs handed in read as released after the failed call


def out_steps(array="null output array", schema="null output schema", cleared=ZEROED):
    return [("out", False, IH, array, cleared), ("out_schema", False, IH, schema, cleared)]


def batch_steps():
    return [("rec", False, IH, "null record batch", ZEROED), ("schema", False, IH, "null record batch", ZEROED)]


def spec_filter_record(e):
    good = dict(expr=e.pred, out=True, out_schema=True, rec=True, schema=True, out_device=CPU)
    steps = [("expr", None, IH, "null expression", ZEROED), *out_steps(), *batch_steps(), ("out_device", 99, IA, OUT_DEVICE, ZEROED)]
    return good, steps, lambda e, v, o, s: e.L.chq_filter_record(e.ctx, *rec_args(e.host, v), None, v["expr"], v["out_device"], o, s)


def spec_filter_records(e):
    good = dict(expr=e.pred, n=1, recs=True, out=True, out_schema=True, out_device=CPU, rec0=True, schema=True)
    steps = [("expr", None, IH, "null expression", ZEROED), ("n", -1, IA, "negative record count", UNTOUCHED),
             ("recs", False, IH, "null record array", ZEROED), *out_steps("null output arrays", "null output schemas"),
             ("out_device", 99, IA, OUT_DEVICE, ZEROED), ("rec0", False, IH, "null record", ZEROED), ("schema", False, IH, "null record batch", ZEROED)]
    return good, steps, lambda e, v, o, s: e.L.chq_filter_records(e.ctx, v["n"], recs_arg(e.host, v), C.pointer(e.host.schema) if v["schema"] else None,
                                                                  None, v["expr"], v["out_device"], o, s)


def spec_filter_records_coalesced(e):
    good = dict(expr=e.pred, out=True, out_schema=True, n=1, recs=True, out_device=CPU, rec0=True, schema=True)
    steps = [("expr", None, IH, "null expression", ZEROED), *out_steps(), ("n", 0, IA, ONE_BATCH, ZEROED), ("recs", False, IH, "null record array", ZEROED),
             ("out_device", 99, IA, OUT_DEVICE, ZEROED), ("rec0", False, IH, "null record", ZEROED), ("schema", False, IH, "null record batch", ZEROED)]
    return good, steps, lambda e, v, o, s: e.L.chq_filter_records_coalesced(
        e.ctx, v["n"], recs_arg(e.host, v), C.pointer(e.host.schema) if v["schema"] else None, None, v["expr"], v["out_device"], o, s, None)


def sort_steps(with_records: bool):
    records = [("n", 0, IA, ONE_BATCH, ZEROED), ("recs", False, IH, "null record array", ZEROED)] if with_records else []
    tail = [("rec0", False, IH, "null record", ZEROED)] if with_records else []
    return [*out_steps(), *records, ("n_keys", -1, IA, "negative sort key count", ZEROED), ("keys", False, IH, "null sort keys", ZEROED),
            ("out_device", 99, IA, OUT_DEVICE, ZEROED), ("key0", None, IH, "null sort key column", ZEROED), *tail,
            ("schema", False, IH, "null record batch", ZEROED)]


def spec_sort_records(e, cb=None):
    cb = cb or e.host
    good = dict(out=True, out_schema=True, n=1, recs=True, n_keys=1, keys=True, out_device=CPU, key0=e.id, rec0=True, schema=True)
    return good, sort_steps(True), lambda e, v, o, s: e.L.chq_sort_records(
        e.ctx, v["n"], recs_arg(cb, v), C.pointer(cb.schema) if v["schema"] else None, None, sort_keys_arg(v), v["n_keys"], -1, v["out_device"], o, s)


def spec_sort_records_device(e):
    return spec_sort_records(e, e.dev)


def spec_sort_record(e):   # (a null record is its own test below: it is reported ahead of everything else)
    good = dict(out=True, out_schema=True, n_keys=1, keys=True, out_device=CPU, key0=e.id, schema=True)
    return good, sort_steps(False), lambda e, v, o, s: e.L.chq_sort_record(
        e.ctx, C.pointer(e.host.array), C.pointer(e.host.schema) if v["schema"] else None, None, sort_keys_arg(v), v["n_keys"], -1, v["out_device"], o, s)


def agg_items_arg(v):
    if not v["items"]:
        return None
    return (_lib.AggItem * 2)(_lib.AggItem(0, 0, None, b"id" if v["name0"] else None), _lib.AggItem(1, 0, None, b"n"))   # KEY 0, COUNT(*)


def aggregate_steps(with_records: bool):
    records = [("n", 0, IA, ONE_BATCH, ZEROED), ("recs", False, IH, "null record array", ZEROED)] if with_records else []
    tail = [("rec0", False, IH, "null record", ZEROED)] if with_records else []
    return [*out_steps(), *records, ("n_keys", -1, IA, "negative GROUP BY key count", ZEROED), ("keys", False, IH, "null GROUP BY keys", ZEROED),
            ("n_items", 0, IA, "GROUP BY needs at least one output item", ZEROED), ("items", False, IH, "null output items", ZEROED),
            ("out_device", 99, IA, OUT_DEVICE, ZEROED), ("key0", None, IH, "null GROUP BY key", ZEROED),
            ("name0", False, IH, "null output column name", ZEROED), *tail, ("schema", False, IH, "null record batch", ZEROED)]


def spec_aggregate_records(e):
    good = dict(out=True, out_schema=True, n=1, recs=True, n_keys=1, keys=True, n_items=2, items=True, out_device=CPU, key0=e.id, name0=True, rec0=True,
                schema=True)
    return good, aggregate_steps(True), lambda e, v, o, s: e.L.chq_aggregate_records(
        e.ctx, v["n"], recs_arg(e.host, v), C.pointer(e.host.schema) if v["schema"] else None, None, exprs_arg(v), v["n_keys"], agg_items_arg(v),
        v["n_items"], v["out_device"], o, s)


def spec_aggregate_record(e):
    good = dict(out=True, out_schema=True, n_keys=1, keys=True, n_items=2, items=True, out_device=CPU, key0=e.id, name0=True, schema=True)
    return good, aggregate_steps(False), lambda e, v, o, s: e.L.chq_aggregate_record(
        e.ctx, C.pointer(e.host.array), C.pointer(e.host.schema) if v["schema"] else None, None, exprs_arg(v), v["n_keys"], agg_items_arg(v),
        v["n_items"], v["out_device"], o, s)


def win_items_arg(v):
    return (_lib.WindowItem * 1)(_lib.WindowItem(0, 0, 0, None, b"rn" if v["name0"] else None)) if v["items"] else None   # ROW_NUMBER


def window_steps(with_records: bool):
    records = [("n", 0, IA, ONE_BATCH, ZEROED), ("recs", False, IH, "null record array", ZEROED)] if with_records else []
    tail = [("rec0", False, IH, "null record", ZEROED)] if with_records else []
    return [*out_steps(), *records, ("n_part", -1, IA, "negative PARTITION BY key count", ZEROED), ("part", False, IH, "null PARTITION BY keys", ZEROED),
            ("n_order", -1, IA, "negative ORDER BY key count", ZEROED), ("order", False, IH, "null ORDER BY keys", ZEROED),
            ("n_items", 0, IA, "a window call needs at least one item", ZEROED), ("items", False, IH, "null window items", ZEROED),
            ("out_device", 99, IA, OUT_DEVICE, ZEROED), ("part0", None, IH, "null PARTITION BY key", ZEROED),
            ("order0", None, IH, "null ORDER BY key column", ZEROED), ("name0", False, IH, "null output column name", ZEROED), *tail,
            ("schema", False, IH, "null record batch", ZEROED)]


def window_tail(v):
    return (exprs_arg(v, "part", "part0"), v["n_part"], sort_keys_arg(v, "order", "order0"), v["n_order"], win_items_arg(v), v["n_items"], v["out_device"])


def spec_window_records(e):
    good = dict(out=True, out_schema=True, n=1, recs=True, n_part=1, part=True, n_order=1, order=True, n_items=1, items=True, out_device=CPU, part0=e.id,
                order0=e.v, name0=True, rec0=True, schema=True)
    return good, window_steps(True), lambda e, v, o, s: e.L.chq_window_records(
        e.ctx, v["n"], recs_arg(e.host, v), C.pointer(e.host.schema) if v["schema"] else None, None, *window_tail(v), o, s)


def spec_window_record(e):
    good = dict(out=True, out_schema=True, n_part=1, part=True, n_order=1, order=True, n_items=1, items=True, out_device=CPU, part0=e.id, order0=e.v,
                name0=True, schema=True)
    return good, window_steps(False), lambda e, v, o, s: e.L.chq_window_record(
        e.ctx, C.pointer(e.host.array), C.pointer(e.host.schema) if v["schema"] else None, None, *window_tail(v), o, s)


def join_spec(e, with_kind: bool):
    good = dict(out=True, out_schema=True, n_left=1, n_right=1, left=True, right=True, left_schema=True, right_schema=True, kind=1, n_keys=1, keys=True,
                out_device=CPU, key_left=e.id, key_right=e.id, left0=True, right0=True)
    per_side = "at least one record batch per side is needed"
    steps = [*out_steps(), ("n_left", 0, IA, per_side, ZEROED), ("n_right", 0, IA, per_side, ZEROED), ("left", False, IH, "null left record array", ZEROED),
             ("right", False, IH, "null right record array", ZEROED), ("left_schema", False, IH, "null left schema", ZEROED),
             ("right_schema", False, IH, "null right schema", ZEROED),
             *([("kind", 99, IA, "unknown join kind 99 (a chq_join_kind is expected)", ZEROED)] if with_kind else []),
             ("n_keys", -1, IA, "negative join key count", ZEROED), ("keys", False, IH, "null join keys", ZEROED), ("out_device", 99, IA, OUT_DEVICE, ZEROED),
             ("key_left", None, IH, "null left join key", ZEROED), ("key_right", None, IH, "null right join key", ZEROED),
             ("left0", False, IH, "null left record", ZEROED), ("right0", False, IH, "null right record", ZEROED)]

    def call(e, v, o, s):
        schema = C.pointer(e.host.schema)
        keys = (_lib.JoinKey * 1)(_lib.JoinKey(v["key_left"], v["key_right"])) if v["keys"] else None
        head = (e.ctx, v["n_left"], recs_arg(e.host, v, "left", "left0"), schema if v["left_schema"] else None, None,
                v["n_right"], recs_arg(e.host, v, "right", "right0"), schema if v["right_schema"] else None, None, keys, v["n_keys"])
        if with_kind:
            return e.L.chq_join_records_kind(*head, v["kind"], v["out_device"], o, s)
        return e.L.chq_join_records(*head, v["out_device"], o, s)
    return good, steps, call


def spec_join_records_kind(e):
    return join_spec(e, True)


def spec_join_records(e):
    return join_spec(e, False)


def spec_partition_records(e):
    good = dict(n=1, recs=True, n_keys=1, keys=True, n_partitions=2, out=True, out_schema=True, out_device=CPU, key0=e.id, rec0=True, schema=True)
    steps = [("n", 0, IA, ONE_BATCH, UNTOUCHED), ("recs", False, IH, "null record array", UNTOUCHED),
             ("n_keys", -1, IA, "negative partition key count", UNTOUCHED), ("keys", False, IH, "null partition keys", UNTOUCHED),
             ("n_partitions", 0, IA, "n_partitions must be in [1, 256] (0 given)", UNTOUCHED),
             *out_steps("null output arrays", "null output schemas", 2), ("out_device", 99, IA, OUT_DEVICE, 2),
             ("key0", None, IH, "null partition key", 2), ("rec0", False, IH, "null record", 2), ("schema", False, IH, "null record batch", 2)]
    return good, steps, lambda e, v, o, s: e.L.chq_partition_records(
        e.ctx, v["n"], recs_arg(e.host, v), C.pointer(e.host.schema) if v["schema"] else None, None, exprs_arg(v), v["n_keys"], v["n_partitions"],
        v["out_device"], o, s)


def select_arg(v):
    return (_lib.SelectItem * 1)(_lib.SelectItem(0, None, None)) if v["fields"] else None   # the wildcard


def spec_project_record(e):
    good = dict(out=True, out_schema=True, fields=True, rec=True, schema=True, out_device=CPU)
    steps = [*out_steps(), ("fields", False, IH, "null select items", ZEROED), *batch_steps(), ("out_device", 99, IA, OUT_DEVICE, ZEROED)]
    return good, steps, lambda e, v, o, s: e.L.chq_project_record(e.ctx, select_arg(v), 1, *rec_args(e.host, v), None, v["out_device"], o, s)


def spec_compute_value(e):   # (a bad out_device is reported last, after the evaluation)
    good = dict(expr=e.pred, out=True, out_schema=True, rec=True, schema=True, out_device=CPU)
    steps = [("expr", None, IH, "null expression", ZEROED), *out_steps(), *batch_steps(), ("out_device", 99, IA, OUT_DEVICE, ZEROED)]
    return good, steps, lambda e, v, o, s: e.L.chq_compute_value(e.ctx, *rec_args(e.host, v), None, v["expr"], v["out_device"], o, s, None)


def spec_filter_project_record(e):
    good = dict(pred=e.pred, out=True, out_schema=True, fields=True, rec=True, schema=True, out_device=CPU)
    steps = [("pred", None, IH, "null predicate", ZEROED), *out_steps(), ("fields", False, IH, "null select items", ZEROED), *batch_steps(),
             ("out_device", 99, IA, OUT_DEVICE, ZEROED)]
    return good, steps, lambda e, v, o, s: e.L.chq_filter_project_record(e.ctx, v["pred"], select_arg(v), 1, *rec_args(e.host, v), None,
                                                                         v["out_device"], o, s)


def spec_record_to_device(e):
    good = dict(out=True, out_schema=True, rec=True, schema=True, resident="host")
    steps = [*out_steps(), *batch_steps(), ("resident", "dev", IA, "record is already device resident", ZEROED)]
    return good, steps, lambda e, v, o, s: e.L.chq_record_to_device(e.ctx, *rec_args(getattr(e, v["resident"]), v), o, s)


def spec_record_to_host(e):
    good = dict(out=True, out_schema=True, rec=True, schema=True, resident="dev")
    steps = [*out_steps(), *batch_steps(), ("resident", "host", IA, "record is already host resident", ZEROED)]
    return good, steps, lambda e, v, o, s: e.L.chq_record_to_host(e.ctx, *rec_args(getattr(e, v["resident"]), v), o, s)


def spec_record_copy_to_peer(e):   # (the "peer" is the same context: one GPU is enough)
    good = dict(out=True, out_schema=True, rec=True, schema=True, resident="dev")
    steps = [*out_steps(), *batch_steps(),
             ("resident", "host", IA, "chq_record_copy_to_peer moves device-resident batches; stage host batches with chq_record_to_device on the "
                                      "destination context", ZEROED)]
    return good, steps, lambda e, v, o, s: e.L.chq_record_copy_to_peer(e.ctx, e.ctx, *rec_args(getattr(e, v["resident"]), v), o, s)


_VALUES = np.arange(3, dtype=np.int32)


def spec_wrap_columns(e):
    good = dict(out=True, out_schema=True, cols=True, format=b"i", values=_VALUES.ctypes.data, null_count=0, offset=0)
    steps = [*out_steps(), ("cols", False, IH, "null column descriptors", ZEROED),
             ("format", b"zz", NS, "Arrow type with format 'zz' is outside this build's scope", ZEROED),
             ("values", None, IA, "column 'x' has no values buffer", ZEROED),
             ("null_count", 1, IA, "column 'x' reports nulls but has no validity bitmap", ZEROED), ("offset", -1, IA, "negative length or offset", ZEROED)]

    def call(e, v, o, s):
        descs = (_lib.ColumnDesc * 1)(_lib.ColumnDesc(b"x", v["format"], 0, v["null_count"], v["offset"], None, v["values"], None)) if v["cols"] else None
        return e.L.chq_wrap_columns(e.ctx, descs, 1, 3, CPU, o, s)
    return good, steps, call


def spec_record_from_ipc(e):
    good = dict(out=True, out_schema=True, stream=e.stream, out_device=CPU, body=None)
    steps = [*out_steps(), ("stream", None, IH, "null stream", ZEROED), ("out_device", 99, IA, OUT_DEVICE, ZEROED),
             ("body", _VALUES.ctypes.data, IA, "body_device_type must be ARROW_DEVICE_CPU or ARROW_DEVICE_ROCM", ZEROED)]
    return good, steps, lambda e, v, o, s: e.L.chq_record_from_ipc(e.ctx, v["stream"], len(e.stream), v["body"], 12, 99, v["out_device"], o, s)


def spec_parquet_read_row_group(e):
    good = dict(out=True, out_schema=True, out_device=CPU, row_group=0)
    steps = [*out_steps(), ("out_device", 99, IA, OUT_DEVICE, ZEROED), ("row_group", 1, IA, "parquet: row group 1 of 1", ZEROED)]
    return good, steps, lambda e, v, o, s: e.L.chq_parquet_read_row_group(e.ctx, e.pq, v["row_group"], v["out_device"], o, s)


def parquet_read_many_spec(e, columns: bool):
    # (only a complete pair of output arrays is cleared)
    good = dict(out=True, out_schema=True, out_device=CPU, first=0)
    steps = [("out", False, IH, "null output arrays", UNTOUCHED), ("out_schema", False, IH, "null output schemas", UNTOUCHED),
             ("out_device", 99, IA, OUT_DEVICE, ZEROED), ("first", 1, IA, "parquet: row groups [1, 2) of 1", ZEROED)]

    def call(e, v, o, s):
        o, s = (None if o is None else vp(o)), (None if s is None else vp(s))
        if columns:
            return e.L.chq_parquet_read_columns(e.ctx, e.pq, v["first"], 1, (C.c_int32 * 1)(0), 1, v["out_device"], o, s)
        return e.L.chq_parquet_read_row_groups(e.ctx, e.pq, v["first"], 1, v["out_device"], o, s)
    return good, steps, call


def spec_parquet_read_columns(e):
    return parquet_read_many_spec(e, True)


def spec_parquet_read_row_groups(e):
    return parquet_read_many_spec(e, False)


SPECS = [spec_filter_record, spec_filter_records, spec_filter_records_coalesced, spec_sort_records, spec_sort_records_device, spec_sort_record,
         spec_aggregate_records, spec_aggregate_record, spec_window_records, spec_window_record, spec_join_records_kind, spec_join_records,
         spec_partition_records, spec_project_record, spec_compute_value, spec_filter_project_record, spec_record_to_device, spec_record_to_host,
         spec_record_copy_to_peer, spec_wrap_columns, spec_record_from_ipc, spec_parquet_read_row_group, spec_parquet_read_columns,
         spec_parquet_read_row_groups]
N_OUT = 2   # output structs behind every `out` / `out_schema` (chq_partition_records writes two)


@pytest.mark.parametrize("spec", SPECS, ids=lambda f: f.__name__[5:])
def test_checks_in_order(env, spec):
    good, steps, call = spec(env)
    v = dict(good)
    for arg, bad, _, _, _ in steps:
        v[arg] = bad
    for i, (arg, _, status, message, after) in enumerate(steps):
        outs, schemas = poisoned(_lib.ArrowDeviceArray, N_OUT), poisoned(_lib.ArrowSchema, N_OUT)
        got = call(env, v, outs if v["out"] else None, schemas if v["out_schema"] else None)
        assert (got, env.error()) == (status, message), f"step {i}: {arg}"
        # what a failed call leaves: nothing to release; the structs it cannot count, and those behind the last, stay as they were
        for name, arr in (("out", outs), ("out_schema", schemas)):
            cleared, size = (after if v[name] else 0), C.sizeof(arr) // N_OUT
            assert bytes(arr) == b"\0" * (cleared * size) + b"\xab" * ((N_OUT - cleared) * size), f"step {i}: {arg}"
        v[arg] = good[arg]
    assert v == good
    outs, schemas = poisoned(_lib.ArrowDeviceArray, N_OUT), poisoned(_lib.ArrowSchema, N_OUT)
    assert call(env, v, outs, schemas) == OK, env.error()
    assert env.error() == ""
    for k in range(2 if spec is spec_partition_records else 1):
        assert outs[k].array.release and schemas[k].release
        release(outs[k].array)
        release(schemas[k])


def test_a_null_record_is_reported_first(env):
    """the *_record forms hand the shared call an array of one: a null record is refused before that, ahead of every other fault"""
    L = env.L
    calls = [lambda o, s: L.chq_sort_record(env.ctx, None, None, None, None, -1, -1, 99, o, s),
             lambda o, s: L.chq_aggregate_record(env.ctx, None, None, None, None, -1, None, 0, 99, o, s),
             lambda o, s: L.chq_window_record(env.ctx, None, None, None, None, -1, None, -1, None, 0, 99, o, s)]
    for call in calls:
        out, schema = poisoned(_lib.ArrowDeviceArray), poisoned(_lib.ArrowSchema)
        assert (call(out, schema), env.error()) == (IH, "null record")
        assert bytes(out) == b"\0" * C.sizeof(out) and bytes(schema) == b"\0" * C.sizeof(schema)
        assert (call(None, None), env.error()) == (IH, "null record")


def test_an_empty_group_filters_to_nothing(env):
    outs, schemas = poisoned(_lib.ArrowDeviceArray), poisoned(_lib.ArrowSchema)
    assert env.L.chq_filter_records(env.ctx, 0, None, None, None, env.pred, 99, outs, schemas) == OK
    assert env.error() == "" and untouched(outs) and untouched(schemas)
    assert env.L.chq_filter_records(env.ctx, 0, None, None, None, env.pred, 99, None, None) == OK


def test_partition_clears_only_a_countable_output_array(env):
    """n_partitions outside [1, kPartMaxPartitions]: the caller's arrays have no known length and stay as they are"""
    recs, keys = (PDA * 1)(C.pointer(env.host.array)), (C.c_void_p * 1)(env.id)
    for p, cleared in ((0, 0), (-3, 0), (MAX_PARTITIONS + 1, 0), (2, 2), (MAX_PARTITIONS, MAX_PARTITIONS)):
        outs, schemas = poisoned(_lib.ArrowDeviceArray, MAX_PARTITIONS + 1), poisoned(_lib.ArrowSchema, MAX_PARTITIONS + 1)
        st = env.L.chq_partition_records(env.ctx, 1, recs, C.pointer(env.host.schema), None, keys, 1, p, 99, outs, schemas)
        assert st == IA
        assert env.error() == (OUT_DEVICE if cleared else f"n_partitions must be in [1, {MAX_PARTITIONS}] ({p} given)")
        for arr in (outs, schemas):
            size = C.sizeof(arr) // (MAX_PARTITIONS + 1)
            assert bytes(arr) == b"\0" * (cleared * size) + b"\xab" * ((MAX_PARTITIONS + 1 - cleared) * size)


def test_parquet_reads_without_a_file(env):
    out, schema = poisoned(_lib.ArrowDeviceArray), poisoned(_lib.ArrowSchema)
    L = env.L
    assert L.chq_parquet_read_row_group(env.ctx, None, 0, CPU, out, schema) == IH
    assert L.chq_parquet_read_row_groups(env.ctx, None, 0, 1, CPU, vp(out), vp(schema)) == IH
    assert L.chq_parquet_read_columns(env.ctx, None, 0, 1, None, -1, CPU, vp(out), vp(schema)) == IH
    assert untouched(out) and untouched(schema)


def test_peer_copy_without_one_of_its_contexts(env):
    out, schema = poisoned(_lib.ArrowDeviceArray), poisoned(_lib.ArrowSchema)
    rec, sch = C.pointer(env.dev.array), C.pointer(env.dev.schema)
    assert env.L.chq_record_copy_to_peer(None, env.ctx, rec, sch, out, schema) == IH
    assert env.L.chq_record_copy_to_peer(env.ctx, None, rec, sch, out, schema) == IH
    assert untouched(out) and untouched(schema)


def test_messages_and_images(env):
    """the entries whose output is a struct of its own: cleared first, then the checks in order"""
    L = env.L
    rec, sch = C.pointer(env.host.array), C.pointer(env.host.schema)
    recs = (PDA * 1)(rec)
    # chq_record_to_ipc
    assert (L.chq_record_to_ipc(env.ctx, None, None, 99, None), env.error()) == (IH, "null output message")
    for args, status, message in (((None, None, 99), IA, "body_device must be ARROW_DEVICE_CPU or ARROW_DEVICE_ROCM"),
                                  ((None, None, CPU), IH, "null record batch"), ((rec, None, CPU), IH, "null record batch")):
        msg = poisoned(_lib.IpcMessage)
        assert (L.chq_record_to_ipc(env.ctx, *args, msg), env.error()) == (status, message)
        assert bytes(msg) == b"\0" * C.sizeof(msg)
    msg = poisoned(_lib.IpcMessage)
    assert L.chq_record_to_ipc(env.ctx, rec, sch, CPU, msg) == OK and env.error() == "" and msg[0].release
    release(msg[0])
    assert bytes(msg) == b"\0" * C.sizeof(msg)
    # chq_record_to_parquet
    assert (L.chq_record_to_parquet(env.ctx, None, None, None), env.error()) == (IH, "null output image")
    for args in ((None, None), (rec, None)):
        img = poisoned(_lib.ParquetImage)
        assert (L.chq_record_to_parquet(env.ctx, *args, img), env.error()) == (IH, "null record batch")
        assert bytes(img) == b"\0" * C.sizeof(img)
    img = poisoned(_lib.ParquetImage)
    assert L.chq_record_to_parquet(env.ctx, rec, sch, img) == OK and env.error() == "" and img[0].release and img[0].len > 8
    release(img[0])
    assert bytes(img) == b"\0" * C.sizeof(img)
    # chq_records_to_parquet
    assert (L.chq_records_to_parquet(env.ctx, 0, None, None, None), env.error()) == (IH, "null output image")
    for args, status, message in (((0, None, None), IH, "null record batches"),
                                  ((0, recs, None), IA, "chq_records_to_parquet needs at least one record batch"),
                                  ((1, (PDA * 1)(), None), IH, "null record batch"), ((1, recs, None), IH, "null record batch")):
        img = poisoned(_lib.ParquetImage)
        assert (L.chq_records_to_parquet(env.ctx, *args, img), env.error()) == (status, message)
        assert bytes(img) == b"\0" * C.sizeof(img)
    img = poisoned(_lib.ParquetImage)
    assert L.chq_records_to_parquet(env.ctx, 1, recs, sch, img) == OK and env.error() == "" and img[0].release
    release(img[0])


def test_set_option_checks(env):
    L = env.L
    assert L.chq_ctx_set_option(env.ctx, None, 0) == IH
    assert (L.chq_ctx_set_option(env.ctx, b"no_such_option", 0), env.error()) == (IA, "unknown option: no_such_option")
    assert (L.chq_ctx_set_option(env.ctx, b"tile_kind", 3), env.error()) == (IA, "tile_kind must be -1..2")
    assert (L.chq_ctx_set_option(env.ctx, b"tile_kind", -1), env.error()) == (OK, "")
