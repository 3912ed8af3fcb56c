"""CPU: ORDER BY without a GPU -- the host reference against pyarrow where the two share semantics (and against totalOrder
where they do not), the ORDER BY / LIMIT parse, and the order-by operator task over the in-process exchange with an
injected host sort."""
import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest

from chapterhouseqe_amd import sqlast as A
from chapterhouseqe_amd.operators import (ExchangeOperator, OperatorInstanceConfig, OrderByOperatorTask, OrderByTaskBuilder,
                                          build_default_operator_task_registry)
from chapterhouseqe_amd.sample_data import simple_batches
from chapterhouseqe_amd.sqlparse import parse_select, parse_statements
from tests import sort_reference as R
from tests.helpers import batches_identical


# ------------------------------------------------------------------------------------------------ the reference
def _arrow_order(batch, keys):
    placement = {nf for _, _, nf in keys}
    assert len(placement) == 1
    where = "at_start" if placement.pop() else "at_end"
    return pc.sort_indices(batch, sort_keys=[(n, "descending" if d else "ascending", where) for n, d, _ in keys]).to_numpy()


@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("nulls_first", [False, True])
def test_reference_agrees_with_arrow_on_shared_semantics(desc, nulls_first):
    rng = np.random.default_rng(3)
    n = 2000
    ints = rng.integers(-50, 50, n)
    strs = ["".join(chr(97 + c) for c in rng.integers(0, 3, rng.integers(0, 4))) for _ in range(n)]
    mask = rng.random(n) < 0.1
    b = pa.RecordBatch.from_arrays([pa.array(ints, type=pa.int64(), mask=mask), pa.array(strs, mask=rng.random(n) < 0.1),
                                    pa.array(rng.integers(0, 1 << 64, n, dtype=np.uint64)), pa.array(np.arange(n, dtype=np.int32))],
                                   names=["i", "s", "u", "row"])
    for keys in ([("i", desc, nulls_first)], [("s", desc, nulls_first)], [("u", desc, nulls_first)],
                 [("s", desc, nulls_first), ("i", not desc, nulls_first)], [("i", desc, nulls_first), ("s", desc, nulls_first)]):
        assert np.array_equal(R.sort_indices(b, keys), _arrow_order(b, keys)), keys


def test_reference_is_stable_and_honours_limit():
    b = pa.RecordBatch.from_arrays([pa.array([2, 1, 2, 1, 2]), pa.array([0, 1, 2, 3, 4])], names=["k", "row"])
    assert R.sort_batch(b, [("k", False, False)]).column(1).to_pylist() == [1, 3, 0, 2, 4]
    assert R.sort_batch(b, [("k", True, False)]).column(1).to_pylist() == [0, 2, 4, 1, 3]
    assert R.sort_batch(b, [("k", False, False)], limit=2).column(1).to_pylist() == [1, 3]


def test_reference_follows_total_order_where_arrow_does_not():
    bits = np.array([0x00000000, 0x80000000, 0x7FC00001, 0xFFC00002, 0x3F800000, 0xFF800000, 0x7F800000, 0x00000001],
                    dtype=np.uint32)   # +0, -0, +NaN, -NaN, 1, -inf, +inf, +subnormal
    b = pa.RecordBatch.from_arrays([pa.array(bits.view(np.float32)), pa.array(np.arange(8, dtype=np.int32))], names=["f", "row"])
    got = bits[R.sort_indices(b, [("f", False, False)])]
    assert got.tolist() == [0xFFC00002, 0xFF800000, 0x80000000, 0x00000000, 0x00000001, 0x3F800000, 0x7F800000, 0x7FC00001]
    assert bits[R.sort_indices(b, [("f", True, False)])].tolist() == got[::-1].tolist()
    arrow = bits[_arrow_order(b, [("f", False, False)])]
    assert arrow.tolist() != got.tolist()     # arrow: -0 == +0 (input order), every NaN last
    assert arrow[:2].tolist() == [0xFF800000, 0x00000000]


def test_reference_orders_utf8_bytewise_with_prefixes_first():
    vals = [b"ab", b"a", b"", b"ab\x00", b"a\x00c", b"\xff", b"abc", b"b"]
    offsets = np.cumsum([0] + [len(v) for v in vals]).astype(np.int32)
    col = pa.Array.from_buffers(pa.utf8(), len(vals), [None, pa.py_buffer(offsets.tobytes()), pa.py_buffer(b"".join(vals))])
    b = pa.RecordBatch.from_arrays([col], names=["s"])
    order = R.sort_indices(b, [("s", False, False)])
    assert [vals[i] for i in order] == sorted(vals)
    assert [vals[i] for i in order][:4] == [b"", b"a", b"a\x00c", b"ab"]


# ------------------------------------------------------------------------------------------------ SQL
def test_parse_order_by_and_limit():
    s = parse_select("select id, value1 from read_files('x') t where id > 3 order by value2 desc nulls last, t.id, value1 asc nulls first limit 10")
    assert s.selection is not None and s.limit == 10
    assert s.order_by == (A.OrderByExpr(A.ident("value2"), False, False), A.OrderByExpr(A.compound("t", "id"), None, None),
                          A.OrderByExpr(A.ident("value1"), True, True))
    assert [o.sort_options() for o in s.order_by] == [(True, False), (False, False), (False, True)]
    plain = parse_select("select id from read_files('x') order by id")
    assert plain.selection is None and plain.limit is None and plain.order_by == (A.OrderByExpr(A.ident("id")),)
    assert parse_select("select id from read_files('x') limit 0").limit == 0


def test_sql_defaults_nulls_last_for_asc_first_for_desc():
    s = parse_select("select a from t order by a, b asc, c desc, d desc nulls last")
    assert [o.sort_options() for o in s.order_by] == [(False, False), (False, False), (True, True), (True, False)]


def test_parse_statements_keeps_order_by_and_limit():
    stmts = parse_statements("select id from read_files('a') where id < 5 order by id desc limit 3;\n"
                             "select * from read_files('b') order by value1, value2 nulls first;")
    assert stmts[0].order_by == (A.OrderByExpr(A.ident("id"), False, None),) and stmts[0].limit == 3
    assert stmts[1].order_by == (A.OrderByExpr(A.ident("value1")), A.OrderByExpr(A.ident("value2"), None, True))
    assert stmts[1].limit is None


def test_select_without_order_by_is_unchanged():
    s = parse_select("select id from read_files('x') where id > 1")
    assert s.order_by == () and s.limit is None
    assert s == type(s)(s.projection, s.from_, s.selection)


def test_order_by_parse_errors():
    from chapterhouseqe_amd.sqlparse import SqlParseError
    for bad in ("select a from t order a", "select a from t order by a nulls middle", "select a from t limit x",
                "select a from t limit 1.5"):
        with pytest.raises(SqlParseError):
            parse_select(bad)


# ------------------------------------------------------------------------------------------------ the operator
def _host_sort(records, aliases, order_by, limit):
    return R.sort_batches(records, R.keys_of(order_by, records[0].schema), limit)


def _run_order_by(batches, order_by, limit=None, max_rows=10_000, sort_fn=_host_sort, max_heartbeat_interval_s=1.0):
    ex_in = ExchangeOperator("operator_p0_exchange", ["operator_p1_producer"], max_heartbeat_interval_s=max_heartbeat_interval_s)
    ex_out = ExchangeOperator("operator_p1_exchange", ["operator_p2_producer"])
    for rid, b in enumerate(batches):
        ex_in.send_record(rid, b, [[] for _ in range(b.num_columns)])
    ex_in.producers_completed()
    task = OrderByOperatorTask(tuple(order_by), limit, max_rows)
    reg = build_default_operator_task_registry("/tmp")
    assert reg.find_task_builder(task) is reg.order_by_task
    run = OrderByTaskBuilder(sort_fn).build(OperatorInstanceConfig(1, "operator_p1_producer", 5, task), [ex_in], ex_out)
    err = run()
    return err, run.task, ex_in, ex_out


def _drain(ex_out):
    ex_out.producers_completed()
    got = []
    while True:
        r = ex_out.get_next_record("operator_p2_producer", 1)
        if not isinstance(r, tuple):
            break
        got.append(r)
        ex_out.operator_completed_record_processing("operator_p2_producer", r[0])
    return got


def test_order_by_task_sends_the_sorted_table_in_record_id_order():
    batches = simple_batches(1000, 4, 33)
    order_by = parse_select("select * from t order by value1 desc, id").order_by
    err, task, ex_in, ex_out = _run_order_by(batches, order_by, max_rows=128)
    assert err is None
    got = _drain(ex_out)
    assert [r[0] for r in got] == list(range(len(got))) and len(got) == 8      # ceil(1000 / 128)
    assert all(r[1].num_rows == 128 for r in got[:-1]) and got[-1][1].num_rows == 1000 - 7 * 128
    exp = R.sort_batches(batches, [("value1", True, True), ("id", False, False)])
    assert batches_identical(R.join([r[1] for r in got]), exp)
    assert ex_in.num_records() == 0 and task.rows_in == 1000 and task.rows_out == 1000


def test_order_by_task_limit():
    batches = simple_batches(300, 4, 33)
    order_by = parse_select("select * from t order by value2").order_by
    err, task, _, ex_out = _run_order_by(batches, order_by, limit=5)
    assert err is None
    got = _drain(ex_out)
    assert len(got) == 1 and batches_identical(got[0][1], R.sort_batches(batches, [("value2", False, False)], 5))


def test_order_by_task_acks_only_after_the_send():
    batches = simple_batches(100, 4, 33)
    seen = []

    class Out(ExchangeOperator):
        def send_record(self, record_id, record, table_aliases):
            seen.append(ex_in.num_records())   # every input still held when the output goes out
            super().send_record(record_id, record, table_aliases)

    ex_in = ExchangeOperator("operator_p0_exchange", ["operator_p1_producer"])
    ex_out = Out("operator_p1_exchange", ["operator_p2_producer"])
    for rid, b in enumerate(batches):
        ex_in.send_record(rid, b, [[] for _ in range(b.num_columns)])
    ex_in.producers_completed()
    task = OrderByOperatorTask(parse_select("select * from t order by id desc").order_by, None, 50)
    run = OrderByTaskBuilder(_host_sort).build(OperatorInstanceConfig(1, "operator_p1_producer", 5, task), [ex_in], ex_out)
    assert run() is None
    assert seen == [len(batches), len(batches)]
    assert ex_in.num_records() == 0


def test_a_failing_sort_leaves_the_inputs_requeueable():
    batches = simple_batches(100, 4, 33)

    def boom(records, aliases, order_by, limit):
        raise RuntimeError("sort failed")

    order_by = parse_select("select * from t order by id").order_by
    err, task, ex_in, ex_out = _run_order_by(batches, order_by, sort_fn=boom, max_heartbeat_interval_s=0.2)
    assert isinstance(err, RuntimeError)
    assert ex_in.num_records() == len(batches) and ex_out.num_records() == 0
    import time
    time.sleep(0.5)
    with ex_in._lock:
        ex_in._pool.maintain()
    q = ex_in._pool.queues[0]
    assert sorted(q.records_to_process) == list(range(len(batches)))     # requeued for another instance
