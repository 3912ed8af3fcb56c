"""CPU: GROUP BY without a GPU -- the host reference pinned to pyarrow's group_by where the two share semantics (and to the
bit-pattern rule where they do not), the GROUP BY parse and the SELECT list -> (keys, items) helper, and the aggregate
operator task over the in-process exchange with the reference injected."""
import math

import numpy as np
import pyarrow as pa
import pytest

from chapterhouseqe_amd import sqlast as A
from chapterhouseqe_amd.operators import (AggregateOperatorTask, AggregateTaskBuilder, ExchangeOperator, OperatorInstanceConfig,
                                          build_default_operator_task_registry)
from chapterhouseqe_amd.sample_data import simple_batches
from chapterhouseqe_amd.sqlparse import SqlParseError, aggregate_plan, parse_expr, parse_select, parse_statements
from tests import aggregate_reference as G
from tests import sort_reference as R
from tests.helpers import batches_identical, explain_diff


# ------------------------------------------------------------------------------------------------ the reference
def _arrow_group_by(batch, keys, value):
    t = pa.Table.from_batches([batch]).group_by(keys, use_threads=False).aggregate(
        [([], "count_all"), (value, "count"), (value, "sum"), (value, "min"), (value, "max")])
    t = t.sort_by([(k, "ascending") for k in keys]).combine_chunks()      # nulls at the end, strings bytewise
    return t.select(keys + ["count_all", f"{value}_count", f"{value}_sum", f"{value}_min", f"{value}_max"])


@pytest.mark.parametrize("keys", [["i"], ["s"], ["s", "i"], ["u", "s"]])
@pytest.mark.parametrize("value", ["v32", "v64", "vu"])
def test_reference_agrees_with_arrow_on_shared_semantics(keys, value):
    rng = np.random.default_rng(11)
    n = 3000
    strs = ["".join(chr(97 + c) for c in rng.integers(0, 3, rng.integers(0, 4))) for _ in range(n)]
    b = pa.RecordBatch.from_arrays([
        pa.array(rng.integers(-6, 6, n), type=pa.int64(), mask=rng.random(n) < 0.1),
        pa.array(strs, mask=rng.random(n) < 0.1),
        pa.array(rng.integers(0, 4, n).astype(np.uint16)),
        pa.array(rng.integers(-2**31, 2**31, n).astype(np.int32), mask=rng.random(n) < 0.3),
        pa.array(rng.integers(-2**50, 2**50, n), type=pa.int64(), mask=rng.random(n) < 0.3),
        pa.array(rng.integers(0, 2**40, n).astype(np.uint64), mask=rng.random(n) < 0.3)], names=["i", "s", "u", "v32", "v64", "vu"])
    items = [("key", k, j) for j, k in enumerate(keys)] + [("count_star", "count_all", None), ("count", f"{value}_count", value),
                                                          ("sum", f"{value}_sum", value), ("min", f"{value}_min", value),
                                                          ("max", f"{value}_max", value)]
    exp, bounds = G.aggregate(b, keys, items)
    arrow = _arrow_group_by(b, keys, value)
    assert not bounds and exp.num_rows == arrow.num_rows > 10
    for c in range(exp.num_columns):
        assert exp.schema.field(c).name == arrow.schema.field(c).name
        assert exp.column(c).to_pylist() == arrow.column(c).to_pylist(), exp.schema.field(c).name
        assert exp.column(c).type == arrow.column(c).type, exp.schema.field(c).name


def test_reference_groups_by_bits_where_arrow_does_not():
    bits = np.array([0x00000000, 0x80000000, 0x7FC00001, 0x7FC00002, 0x00000000, 0x7FC00001, 0x80000000], dtype=np.uint32)
    b = pa.RecordBatch.from_arrays([pa.array(bits.view(np.float32)), pa.array(np.arange(7, dtype=np.int32))], names=["f", "row"])
    exp, _ = G.aggregate(b, ["f"], [("key", "f", 0), ("count_star", "n", None), ("min", "first", "row")])
    # totalOrder: -0 < +0 < NaN(payload 1) < NaN(payload 2)
    assert exp.column(0).to_numpy().view(np.uint32).tolist() == [0x80000000, 0x00000000, 0x7FC00001, 0x7FC00002]
    assert exp.column(1).to_pylist() == [2, 2, 2, 1] and exp.column(2).to_pylist() == [1, 0, 2, 3]


def test_reference_zero_keys_and_zero_rows():
    b = pa.RecordBatch.from_arrays([pa.array([], type=pa.int32()), pa.array([], type=pa.float32())], names=["k", "v"])
    items = [("count_star", "n", None), ("count", "c", "v"), ("sum", "s", "v"), ("min", "lo", "k")]
    exp, _ = G.aggregate(b, [], items)
    assert exp.to_pylist() == [{"n": 0, "c": 0, "s": None, "lo": None}]
    assert [f.nullable for f in exp.schema] == [False, False, True, True]
    assert G.aggregate(b, ["k"], [("key", "k", 0)] + items)[0].num_rows == 0


def test_reference_integer_overflow_is_decided_on_the_exact_total():
    big = 2**63 - 1
    b = pa.RecordBatch.from_arrays([pa.array([big, 1, -5], type=pa.int64())], names=["v"])
    assert G.aggregate(b, [], [("sum", "s", "v")])[0].column(0).to_pylist() == [big - 4]
    with pytest.raises(G.SumOverflow):
        G.aggregate(b.slice(0, 2), [], [("sum", "s", "v")])


def test_reference_float_sums_follow_ieee_on_non_finite_values():
    assert math.isnan(G.float_sum(np.array([1.0, math.nan]))) and math.isnan(G.float_sum(np.array([math.inf, -math.inf, 1.0])))
    assert G.float_sum(np.array([math.inf, 1e308, 1e308])) == math.inf and G.float_sum(np.array([-math.inf, 3.0])) == -math.inf
    assert G.float_sum(np.array([1e100, 1.0, -1e100])) == 1.0        # exact, whatever the order


# ------------------------------------------------------------------------------------------------ SQL
def test_parse_group_by_between_where_and_order_by():
    s = parse_select("select value1, count(*), sum(value2) from read_files('x') t where id > 3 group by value1, t.id "
                     "order by value1 desc limit 7")
    assert s.group_by == (A.ident("value1"), A.compound("t", "id"))
    assert s.selection is not None and s.limit == 7 and s.order_by == (A.OrderByExpr(A.ident("value1"), False, None),)
    assert parse_select("select a from t").group_by == ()
    s2 = parse_statements("select a, max(b) from read_files('x') group by a; select a from read_files('y')")
    assert s2[0].group_by == (A.ident("a"),) and s2[1].group_by == ()
    with pytest.raises(SqlParseError):
        parse_select("select a from t group a")


def test_select_positional_construction_still_works():
    s = parse_select("select id from read_files('x') where id > 1")
    assert s == type(s)(s.projection, s.from_, s.selection) == type(s)(s.projection, s.from_, s.selection, (), None)


def test_function_calls_stay_unsupported_expressions_for_the_evaluator():
    e = parse_expr("abs(a)")
    assert isinstance(e, A.UnsupportedExpr) and isinstance(e, A.Function) and e.debug == "Function(abs)"
    assert (e.name, e.args, e.star) == ("abs", (A.ident("a"),), False)
    c = parse_expr("COUNT(*)")
    assert isinstance(c, A.UnsupportedExpr) and (c.name, c.args, c.star, c.debug) == ("COUNT", (), True, "Function(COUNT)")
    assert parse_expr("f(a, b + 1)").args == (A.ident("a"), A.binop(A.ident("b"), A.BinaryOperator.Plus, A.number("1")))
    assert parse_expr("cast(a as int)").args is None and parse_expr("now()").args == ()
    # the text an enclosing unsupported node quotes is what it was before calls carried their arguments
    assert parse_expr("-abs(a)").debug == "UnaryOp { op: Minus, expr: UnsupportedExpr(debug='Function(abs)') }"


def test_aggregate_plan_names_and_aliases():
    s = parse_select("select value1, COUNT(*), Sum(value2) as total, min(t.id), max(id) biggest, count(value2), value1 as again "
                     "from read_files('x') t group by value1")
    keys, items = aggregate_plan(s)
    assert keys == (A.ident("value1"),)
    assert items == (A.AggItem(A.AggKind.KEY, "value1", 0),
                     A.AggItem(A.AggKind.COUNT_STAR, "count(*)"),
                     A.AggItem(A.AggKind.SUM, "total", -1, A.ident("value2")),
                     A.AggItem(A.AggKind.MIN, "min(t.id)", -1, A.compound("t", "id")),
                     A.AggItem(A.AggKind.MAX, "biggest", -1, A.ident("id")),
                     A.AggItem(A.AggKind.COUNT, "count(value2)", -1, A.ident("value2")),
                     A.AggItem(A.AggKind.KEY, "again", 0))
    assert G.from_plan(keys, items) == (["value1"], [("key", "value1", 0), ("count_star", "count(*)", None), ("sum", "total", "value2"),
                                                    ("min", "min(t.id)", "id"), ("max", "biggest", "id"),
                                                    ("count", "count(value2)", "value2"), ("key", "again", 0)])


def test_aggregate_plan_without_keys_and_without_aggregates():
    keys, items = aggregate_plan(parse_select("select sum(a), count(*) n from t"))
    assert keys == () and [i.kind for i in items] == [A.AggKind.SUM, A.AggKind.COUNT_STAR] and items[1].name == "n"
    keys, items = aggregate_plan(parse_select("select b from t group by a, b"))      # a key need not be selected
    assert keys == (A.ident("a"), A.ident("b")) and items == (A.AggItem(A.AggKind.KEY, "b", 1),)
    assert aggregate_plan(parse_select("select a, abs(b) from t where a > 1 order by a")) is None


@pytest.mark.parametrize("sql", [
    "select a, b, count(*) from t group by a",            # a stray column
    "select a, abs(b) from t group by a",                 # a call that is no aggregate
    "select a + 1, count(*) from t group by a",           # an expression
    "select *, count(*) from t group by a",
    "select sum(*) from t",
    "select sum(a, b) from t",
    "select count() from t",
    "select count(distinct a) from t",
])
def test_aggregate_plan_errors(sql):
    with pytest.raises(SqlParseError):
        aggregate_plan(parse_select(sql))


# ------------------------------------------------------------------------------------------------ the operator
def _host_aggregate(records, aliases, keys, items):
    rk, ri = G.from_plan(keys, items)
    return G.aggregate_batches(records, rk, ri)[0]


def _run_aggregate(batches, sql, max_rows=10_000, aggregate_fn=_host_aggregate, out_cls=ExchangeOperator):
    keys, items = aggregate_plan(parse_select(sql))
    ex_in = ExchangeOperator("operator_p0_exchange", ["operator_p1_producer"])
    ex_out = out_cls("operator_p1_exchange", ["operator_p2_producer"])
    for rid, b in enumerate(batches):
        ex_in.send_record(rid, b, [[] for _ in range(b.num_columns)])
    ex_in.producers_completed()
    task = AggregateOperatorTask(keys, items, max_rows)
    reg = build_default_operator_task_registry("/tmp")
    assert reg.find_task_builder(task) is reg.aggregate_task
    run = AggregateTaskBuilder(aggregate_fn).build(OperatorInstanceConfig(1, "operator_p1_producer", 5, task), [ex_in], ex_out)
    return run(), run.task, ex_in, ex_out


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


def test_aggregate_task_sends_the_groups_in_key_order():
    batches = simple_batches(1000, 4, 33)
    sql = "select value1, count(*), sum(value2) as total, min(id) from t group by value1"
    err, task, ex_in, ex_out = _run_aggregate(batches, sql, max_rows=100)
    assert err is None
    got = _drain(ex_out)
    exp = _host_aggregate(batches, None, *aggregate_plan(parse_select(sql)))
    assert exp.schema.names == ["value1", "count(*)", "total", "min(id)"] and exp.num_rows > 100
    assert [r[0] for r in got] == list(range(len(got))) and len(got) == -(-exp.num_rows // 100)
    assert all(len(r[2]) == 4 for r in got)                                # one (empty) alias list per output column
    joined = R.join([r[1] for r in got])
    assert batches_identical(joined, exp), explain_diff(joined, exp)
    assert ex_in.num_records() == 0 and task.rows_in == 1000 and task.rows_out == exp.num_rows
    keys = joined.column(0).to_pylist()
    assert keys == sorted(keys)


def test_aggregate_task_without_keys_sends_one_row():
    batches = simple_batches(300, 4, 33)
    err, task, _, ex_out = _run_aggregate(batches, "select count(*) n, max(id) top from t")
    assert err is None
    got = _drain(ex_out)
    assert len(got) == 1 and got[0][1].to_pylist() == [{"n": 300, "top": max(max(b.column(0).to_pylist()) for b in batches)}]


def test_aggregate_task_acks_only_after_the_send():
    batches = simple_batches(100, 4, 33)
    seen = []
    holder = {}

    class Out(ExchangeOperator):
        def send_record(self, record_id, record, table_aliases):
            seen.append(holder["ex_in"].num_records())   # every input still held when the output goes out
            super().send_record(record_id, record, table_aliases)

    keys, items = aggregate_plan(parse_select("select id, count(*) from t group by id"))
    ex_in = ExchangeOperator("operator_p0_exchange", ["operator_p1_producer"])
    holder["ex_in"] = ex_in
    ex_out = Out("operator_p1_exchange", ["operator_p2_producer"])
    for rid, b in enumerate(batches):
        ex_in.send_record(rid, b, [[] for _ in range(b.num_columns)])
    ex_in.producers_completed()
    task = AggregateOperatorTask(keys, items, 50)
    run = AggregateTaskBuilder(_host_aggregate).build(OperatorInstanceConfig(1, "operator_p1_producer", 5, task), [ex_in], ex_out)
    assert run() is None
    assert seen == [len(batches), len(batches)]
    assert ex_in.num_records() == 0


def test_a_failing_aggregate_keeps_the_inputs_unacked():
    batches = simple_batches(100, 4, 33)

    def boom(records, aliases, keys, items):
        raise RuntimeError("aggregate failed")

    err, task, ex_in, ex_out = _run_aggregate(batches, "select count(*) from t", aggregate_fn=boom)
    assert isinstance(err, RuntimeError)
    assert ex_in.num_records() == len(batches) and ex_out.num_records() == 0
