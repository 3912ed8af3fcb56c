"""CPU: AVG, COUNT(DISTINCT), HAVING and SELECT DISTINCT without a GPU -- the host reference of tests/aggregate_ext_reference.py
pinned to pyarrow and sqlite3 where they share semantics, the grammar, `having_plan`, the aggregate operator task with HAVING
over the in-process exchange with host functions injected, and avg_rn.h alone in a stand-alone program under the address and
undefined-behaviour sanitizers."""
import os
import shutil
import sqlite3
import subprocess

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest

from chapterhouseqe_amd import sqlast as A
from chapterhouseqe_amd.operators import (AggregateOperatorTask, AggregateTaskBuilder, ExchangeOperator, OperatorInstanceConfig,
                                          build_default_operator_task_registry)
from chapterhouseqe_amd.sample_data import simple_batches
from chapterhouseqe_amd.sqlparse import (Select, SqlParseError, aggregate_plan, having_plan, parse_select, parse_statements,
                                         window_plan)
from oracle import oracle as O
from tests import aggregate_ext_reference as X
from tests import sort_reference as R
from tests.helpers import batches_identical, explain_diff

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the reference
def _table(rng, n):
    strs = ["".join(chr(97 + c) for c in rng.integers(0, 3, rng.integers(0, 4))) for _ in range(n)]
    return pa.RecordBatch.from_arrays([
        pa.array(rng.integers(-6, 6, n), type=pa.int64(), mask=rng.random(n) < 0.1),
        pa.array(strs, mask=rng.random(n) < 0.1),
        pa.array(rng.integers(-2**31, 2**31, n).astype(np.int32), mask=rng.random(n) < 0.3),
        pa.array(rng.integers(0, 2**40, n).astype(np.uint64), mask=rng.random(n) < 0.3),
        pa.array(rng.integers(-1000, 1000, n).astype(np.float64), mask=rng.random(n) < 0.3),
        pa.array(rng.integers(-9, 9, n).astype(np.int16), mask=rng.random(n) < 0.3),
        pa.array([strs[i] for i in rng.integers(0, n, n)], mask=rng.random(n) < 0.3)], names=["i", "s", "v32", "vu", "vf", "d", "ds"])


@pytest.mark.parametrize("keys", [["i"], ["s"], ["s", "i"]])
@pytest.mark.parametrize("value", ["v32", "vu", "vf"])
def test_avg_agrees_with_arrow_mean_where_the_total_is_exact(keys, value):
    """integer-valued data whose group totals stay below 2^53: arrow's mean (a double sum over the count) is then exactly
    RN(T) / count too"""
    b = _table(np.random.default_rng(12), 3000)
    exp, _ = X.aggregate(b, keys, [("key", k, j) for j, k in enumerate(keys)] + [("avg", "m", value), ("count", "c", value)])
    t = pa.Table.from_batches([b]).group_by(keys, use_threads=False).aggregate([(value, "mean")])
    t = t.sort_by([(k, "ascending") for k in keys]).combine_chunks()
    assert exp.num_rows == t.num_rows > 10
    assert exp.column("m").to_pylist() == t.column(f"{value}_mean").to_pylist()
    assert exp.column("m").type == pa.float64() and exp.schema.field("m").nullable
    assert [m is None for m in exp.column("m").to_pylist()] == [c == 0 for c in exp.column("c").to_pylist()]


@pytest.mark.parametrize("keys", [["i"], ["s", "i"], []])
@pytest.mark.parametrize("value", ["d", "ds", "v32"])
def test_count_distinct_agrees_with_arrow_on_integers_and_strings(keys, value):
    """(float zeros and NaNs are deliberately NOT pinned to arrow: it counts -0 and +0 as one value and all NaNs as one, the
    reference counts bit patterns, like the keys -- the next test)"""
    b = _table(np.random.default_rng(13), 3000)
    exp, _ = X.aggregate(b, keys, [("key", k, j) for j, k in enumerate(keys)] + [("count_distinct", "n", value)])
    if keys:
        t = pa.Table.from_batches([b]).group_by(keys, use_threads=False).aggregate([(value, "count_distinct", pc.CountOptions(mode="only_valid"))])
        t = t.sort_by([(k, "ascending") for k in keys]).combine_chunks()
        want = t.column(f"{value}_count_distinct").to_pylist()
    else:
        want = [pc.count_distinct(b.column(value), mode="only_valid").as_py()]
    assert exp.column("n").to_pylist() == want and exp.num_rows == len(want)
    assert exp.column("n").type == pa.int64() and not exp.schema.field("n").nullable


def test_count_distinct_counts_bit_patterns():
    bits = np.array([0x00000000, 0x80000000, 0x7FC00001, 0x7FC00002, 0x00000000, 0x7FC00001, 0x3F800000], dtype=np.uint32)
    b = pa.RecordBatch.from_arrays([pa.array(bits.view(np.float32), mask=np.array([0, 0, 0, 0, 0, 0, 1], bool)),
                                    pa.array(["a", "ab", "a", None, "", "ab", "abc"])], names=["f", "s"])
    exp, _ = X.aggregate(b, [], [("count_distinct", "nf", "f"), ("count_distinct", "ns", "s")])
    assert exp.to_pylist() == [{"nf": 4, "ns": 4}]                     # -0, +0, two NaN payloads; "a", "ab", "", "abc"
    empty = b.slice(0, 0)
    assert X.aggregate(empty, [], [("count_distinct", "n", "f"), ("avg", "m", "f")])[0].to_pylist() == [{"n": 0, "m": None}]
    assert X.aggregate(empty, ["s"], [("count_distinct", "n", "f")])[0].num_rows == 0


def test_avg_of_integers_rounds_the_exact_total_once_and_never_overflows():
    big = 2**63 - 1
    b = pa.RecordBatch.from_arrays([pa.array([big, big], type=pa.int64()), pa.array([2**64 - 1, 2**11 + 2], type=pa.uint64())], names=["v", "u"])
    exp, _ = X.aggregate(b, [], [("avg", "m", "v"), ("avg", "mu", "u")])
    assert exp.column(0).to_pylist() == [9.223372036854775807e18]
    assert exp.column(1).to_pylist() == [float(2**64 + 2**11 + 1) / 2.0] and float(2**64 + 2**11 + 1) > 2.0**64


def test_avg_of_floats_follows_ieee_on_non_finite_values():
    inf, nan = float("inf"), float("nan")
    b = pa.RecordBatch.from_arrays([pa.array([0, 0, 1, 1, 2, 2, 3], type=pa.int32()), pa.array([1.0, nan, inf, -inf, inf, 1.0, None])], names=["k", "v"])
    got = X.aggregate(b, ["k"], [("avg", "m", "v")])[0].column(0).to_pylist()
    assert np.isnan(got[0]) and np.isnan(got[1]) and got[2] == inf and got[3] is None


def test_reference_agrees_with_sqlite_on_small_integer_tables():
    rng = np.random.default_rng(14)
    n = 2000
    k = [None if rng.random() < 0.05 else int(x) for x in rng.integers(0, 40, n)]
    v = [None if rng.random() < 0.3 else int(x) for x in rng.integers(-50, 50, n)]
    b = pa.RecordBatch.from_arrays([pa.array(k, type=pa.int32()), pa.array(v, type=pa.int64())], names=["k", "v"])
    db = sqlite3.connect(":memory:")
    db.execute("create table t (k integer, v integer)")
    db.executemany("insert into t values (?, ?)", list(zip(k, v)))
    items = [("key", "k", 0), ("avg", "m", "v"), ("count_distinct", "d", "v"), ("count_star", "n", None)]
    exp, _ = X.aggregate(b, ["k"], items)
    rows = db.execute("select k, avg(v), count(distinct v), count(*) from t group by k order by k is null, k").fetchall()
    assert [tuple(r.values()) for r in exp.to_pylist()] == rows and len(rows) == 41
    kept = X.having(exp, lambda r: None if r["m"] is None else r["n"] > 45 and r["m"] < 1.5)
    rows = db.execute("select k, avg(v), count(distinct v), count(*) from t group by k having count(*) > 45 and avg(v) < 1.5 "
                      "order by k is null, k").fetchall()
    assert [tuple(r.values()) for r in kept.to_pylist()] == rows and 0 < len(rows) < 41
    assert X.aggregate(b, [], items[1:])[0].to_pylist() == [dict(zip(["m", "d", "n"], db.execute("select avg(v), count(distinct v), count(*) from t").fetchone()))]


def test_plan_round_trip_of_the_new_kinds():
    keys, items = X.to_plan(["k"], [("key", "k", 0), ("avg", "m", "v"), ("count_distinct", "d", "w"), ("sum", "s", "v")])
    assert items == [A.AggItem(A.AggKind.KEY, "k", 0), A.AggItem(A.AggKind.AVG, "m", -1, A.ident("v")),
                     A.AggItem(A.AggKind.COUNT_DISTINCT, "d", -1, A.ident("w")), A.AggItem(A.AggKind.SUM, "s", -1, A.ident("v"))]
    assert X.from_plan(keys, items) == (["k"], [("key", "k", 0), ("avg", "m", "v"), ("count_distinct", "d", "w"), ("sum", "s", "v")])
    assert (int(A.AggKind.AVG), int(A.AggKind.COUNT_DISTINCT)) == (6, 7)


# ------------------------------------------------------------------------------------------------ SQL
GT1 = A.binop(A.ident("count(*)"), A.BinaryOperator.Gt, A.number("1"))


def test_having_parses_between_group_by_and_order_by():
    s = parse_select("select value1, avg(value2), count(*) from t group by value1 having count(*) > 1")
    assert s.group_by == (A.ident("value1"),) and s.having is not None and s.order_by == () and s.limit is None
    s = parse_select("select a, count(*) from read_files('x') t where a > 3 group by a having count(*) > 1 order by a desc limit 7")
    assert s.selection is not None and s.group_by == (A.ident("a"),) and s.limit == 7
    assert s.order_by == (A.OrderByExpr(A.ident("a"), False, None),)
    assert having_plan(s)[2] == GT1
    assert parse_select("select count(*) from t having count(*) > 1 limit 2").limit == 2            # without GROUP BY
    assert parse_select("select count(*) from t where a > 1 having count(*) > 1 order by 1").selection is not None
    assert parse_select("select a from t group by a").having is None and parse_select("select a from t").having is None
    s2 = parse_statements("select a, max(b) from t group by a having max(b) > 2; select a from u")
    assert s2[0].having is not None and s2[1].having is None
    for bad in ("select a from t having count(*) > 1 group by a",             # HAVING stands behind GROUP BY
                "select a from t having count(*) > 1 where a > 1",
                "select a from t group by a order by a having count(*) > 1",
                "select a from t group by a limit 3 having count(*) > 1",
                "select a from t group by a having"):
        with pytest.raises(SqlParseError):
            parse_select(bad)


def test_having_ends_an_alias_position():
    s = parse_select("select count(*) n from read_files('x') having count(*) > 1")
    assert s.from_.alias is None and s.having is not None
    s = parse_select("select count(*) n from read_files('x') t having count(*) > 1")
    assert s.from_.alias == "t" and s.having is not None
    s = parse_select("select a b, count(*) c from t group by a having c > 1")
    assert [f.alias.value for f in s.projection] == ["b", "c"]
    assert parse_select('select a as "having" from t').projection[0].alias.value == "having"       # behind AS it still is one


def test_select_distinct_forms():
    s = parse_select("select distinct a, t.b x from read_files('p') t where a > 1 order by a limit 5")
    assert s.distinct and s.limit == 5 and len(s.projection) == 2
    assert aggregate_plan(s) == ((A.ident("a"), A.compound("t", "b")), (A.AggItem(A.AggKind.KEY, "a", 0), A.AggItem(A.AggKind.KEY, "x", 1)))
    assert aggregate_plan(parse_select("select distinct t.b from t")) == ((A.compound("t", "b"),), (A.AggItem(A.AggKind.KEY, "b", 0),))
    assert parse_select("select distinct * from t").distinct and parse_select("select DISTINCT (a) from t").distinct
    assert parse_select('select distinct "a" from t').distinct and parse_select("select distinct 1 from t").distinct
    plain = parse_select("select a from t")
    assert not plain.distinct and aggregate_plan(plain) is None


def test_distinct_stays_a_column_name_where_no_expression_follows():
    s = parse_select("select distinct from t")
    assert not s.distinct and s.projection == (A.UnnamedExpr(A.ident("distinct")),) and s.from_.func_name == "t"
    s = parse_select("select distinct, a from t")
    assert not s.distinct and s.projection[0] == A.UnnamedExpr(A.ident("distinct"))
    s = parse_select("select distinct as d from t")
    assert not s.distinct and s.projection[0].alias.value == "d"
    assert not parse_select("select a distinct from t").distinct                                   # an alias


@pytest.mark.parametrize("sql", [
    "select distinct * from t",
    "select distinct t.* from t",
    "select distinct a + 1 from t",
    "select distinct abs(a) from t",
    "select distinct a from t group by a",
    "select distinct a, count(*) from t",
    "select distinct sum(a) from t",
    "select distinct a, rank() over (order by a) from t",
    "select distinct a from t having a > 1",
])
def test_select_distinct_errors(sql):
    with pytest.raises(SqlParseError):
        aggregate_plan(parse_select(sql))


def test_avg_joins_the_aggregates():
    keys, items = aggregate_plan(parse_select("select avg(b) from t"))
    assert keys == () and items == (A.AggItem(A.AggKind.AVG, "avg(b)", -1, A.ident("b")),)
    keys, items = aggregate_plan(parse_select("select a, AVG(t.b) as mean, avg(b) from t group by a"))
    assert items[1:] == (A.AggItem(A.AggKind.AVG, "mean", -1, A.compound("t", "b")), A.AggItem(A.AggKind.AVG, "avg(b)", -1, A.ident("b")))
    for bad in ("select avg(*) from t", "select avg(a, b) from t", "select avg() from t", "select avg(distinct a) from t"):
        with pytest.raises(SqlParseError):
            aggregate_plan(parse_select(bad))


def test_spellings_that_stay_errors():
    with pytest.raises(SqlParseError):
        aggregate_plan(parse_select("select count(distinct a) from t"))
    with pytest.raises(SqlParseError):
        having_plan(parse_select("select a from t group by a having count(distinct b) > 1"))
    for sql in ("select avg(a) over (order by a) from t", "select count(distinct a) over (order by a) from t"):
        with pytest.raises(SqlParseError):
            window_plan(parse_select(sql))


def test_aggregate_plan_ignores_having():
    with_h = parse_select("select a, sum(b) from t group by a having sum(b) > 1 and min(c) < 2")
    without = parse_select("select a, sum(b) from t group by a")
    assert aggregate_plan(with_h) == aggregate_plan(without) and len(aggregate_plan(with_h)) == 2
    assert having_plan(without) is None


def test_having_plan_reuses_visible_items_and_appends_hidden_ones():
    s = parse_select("select value1, avg(value2), count(*) from t group by value1 having count(*) > 1")
    keys, items, pred, n_visible = having_plan(s)
    assert (keys, items) == aggregate_plan(s) and n_visible == 3 and pred == GT1                    # everything reused
    s = parse_select("select a, sum(b) total from t group by a, c having sum(b) > 1 and (min(b) < 2 or c = 3) and a is not null and min(b) > 0")
    keys, items, pred, n_visible = having_plan(s)
    assert keys == (A.ident("a"), A.ident("c")) and n_visible == 2 and items[:2] == aggregate_plan(s)[1]
    assert items[2:] == (A.AggItem(A.AggKind.MIN, "__having_0", -1, A.ident("b")), A.AggItem(A.AggKind.KEY, "__having_1", 1))
    gt, lt, eq = A.BinaryOperator.Gt, A.BinaryOperator.Lt, A.BinaryOperator.Eq
    And, Or = A.BinaryOperator.And, A.BinaryOperator.Or
    assert pred == A.binop(A.binop(A.binop(A.binop(A.ident("total"), gt, A.number("1")), And,
                                           A.Nested(A.binop(A.binop(A.ident("__having_0"), lt, A.number("2")), Or,
                                                            A.binop(A.ident("__having_1"), eq, A.number("3"))))), And,
                                   A.IsNull(A.ident("a"), True)), And, A.binop(A.ident("__having_0"), gt, A.number("0")))
    # an argument spelled differently is another item; COUNT(*) and COUNT(c) differ; avg is an aggregate of HAVING too
    _, items, pred, n_visible = having_plan(parse_select("select count(b) from t having count(*) > 1 and avg(t.b) between 1 and 2"))
    assert n_visible == 1 and [(i.kind, i.name, i.column) for i in items[1:]] == [
        (A.AggKind.COUNT_STAR, "__having_0", None), (A.AggKind.AVG, "__having_1", A.compound("t", "b"))]
    assert pred.right == A.Between(A.ident("__having_1"), False, A.number("1"), A.number("2"))


def test_having_plan_duplicate_output_names_force_a_hidden_item():
    s = parse_select("select a, count(*) as x, sum(b) as x from t group by a having count(*) > 1 and sum(b) > 2 and a > 0")
    _, items, pred, n_visible = having_plan(s)
    assert n_visible == 3 and [(i.kind, i.name) for i in items[3:]] == [(A.AggKind.COUNT_STAR, "__having_0"), (A.AggKind.SUM, "__having_1")]
    assert pred.right == A.binop(A.ident("a"), A.BinaryOperator.Gt, A.number("0"))                  # the key's name is unique
    # a visible column that already has a hidden item's name pushes the number on
    _, items, _, _ = having_plan(parse_select("select a as __having_0 from t group by a having count(*) > 1"))
    assert [i.name for i in items] == ["__having_0", "__having_1"]


@pytest.mark.parametrize("sql", [
    "select a from t group by a having b > 1",                           # an identifier that is no key
    "select a from t group by a having sum(b + 1) > 1",                  # an aggregate of an expression
    "select a from t group by a having sum(b, c) > 1",
    "select a from t group by a having sum(*) > 1",
    "select a from t group by a having rank() over (order by a) > 1",   # a window call
    "select a from t having a > 1",                                      # neither GROUP BY nor an aggregate
    "select 1 from t having count(*) > 1",                               # an aggregate in HAVING alone does not group the statement
    "select a from t having count(*) > 1",
    "select a, rank() over (order by a) from t having a > 1",
])
def test_having_plan_errors(sql):
    with pytest.raises(SqlParseError):
        having_plan(parse_select(sql))


def test_positional_construction_still_works():
    s = parse_select("select id from read_files('x') where id > 1")
    assert s == Select(s.projection, s.from_, s.selection) == Select(s.projection, s.from_, s.selection, (), None, (), ())
    assert Select(s.projection, s.from_, s.selection, (), None, (), (), GT1, True).distinct
    t = AggregateOperatorTask((), (A.AggItem(A.AggKind.COUNT_STAR, "n"),), 50)
    assert (t.max_rows_per_record, t.having, t.n_visible) == (50, None, None)


# ------------------------------------------------------------------------------------------------ the operator
def _batches(n=1000, parts=4, pool=60):
    """the sample schema with value1 drawn from `pool` strings, so that groups have several rows"""
    rng = np.random.default_rng(33)
    names = ["".join(chr(97 + c) for c in rng.integers(0, 26, 4)) for _ in range(pool)]
    out = []
    for p in range(parts):
        m = n // parts
        out.append(pa.RecordBatch.from_arrays([pa.array(np.arange(p * m, (p + 1) * m, dtype=np.int32)),
                                               pa.array([names[i] for i in np.minimum(rng.integers(0, 2 * pool, m), pool - 1 - rng.integers(0, pool, m) % 7)]),
                                               pa.array((rng.random(m) * 100).astype(np.float32), mask=rng.random(m) < 0.1)],
                                              names=["id", "value1", "value2"]))
    return out


def _as_projected(batch):
    """the schema a pass-through projection gives: a column without a null comes out as not nullable (the evaluator's rule)"""
    fields = [pa.field(f.name, f.type, batch.column(i).null_count > 0) for i, f in enumerate(batch.schema)]
    return pa.RecordBatch.from_arrays(batch.columns, schema=pa.schema(fields))


def _host_aggregate(records, aliases, keys, items):
    return X.aggregate_batches(records, *X.from_plan(keys, items))[0]


def _run(batches, sql, max_rows=10_000, **fns):
    sel = parse_select(sql)
    keys, items, pred, n_visible = having_plan(sel)
    ex_in = ExchangeOperator("operator_p0_exchange", ["operator_p1_producer"])
    ex_out = ExchangeOperator("operator_p1_exchange", ["operator_p2_producer"])
    for rid, b in enumerate(batches):
        ex_in.send_record(rid, b, [[] for _ in range(b.num_columns)])
    ex_in.producers_completed()
    task = AggregateOperatorTask(keys, items, max_rows, pred, n_visible)
    reg = build_default_operator_task_registry("/tmp")
    assert reg.find_task_builder(task) is reg.aggregate_task
    run = AggregateTaskBuilder(_host_aggregate, **fns).build(OperatorInstanceConfig(1, "operator_p1_producer", 5, task), [ex_in], ex_out)
    err = run()
    ex_out.producers_completed()
    got = []
    while True:
        r = ex_out.get_next_record("operator_p2_producer", 1)
        if not isinstance(r, tuple):
            break
        got.append(r)
        ex_out.operator_completed_record_processing("operator_p2_producer", r[0])
    return err, run.task, ex_in, got, (keys, items, n_visible)


def _calls(log, name, fn):
    def wrapped(*args):
        log.append(name)
        return fn(*args)
    return wrapped


def test_aggregate_task_with_having_over_visible_items():
    batches = _batches()
    log = []
    err, task, ex_in, got, (keys, items, n_visible) = _run(
        batches, "select value1, avg(value2), count(*) from t group by value1 having count(*) > 12", max_rows=10,
        filter_fn=_calls(log, "filter", O.filter_record), project_fn=_calls(log, "project", O.project_record))
    assert err is None and log == ["filter"] and n_visible == len(items) == 3                      # nothing hidden: no projection
    full = _host_aggregate(batches, None, keys, items)
    exp = X.having(full, lambda r: r["count(*)"] > 12)
    joined = R.join([r[1] for r in got])
    assert batches_identical(joined, exp), explain_diff(joined, exp)
    assert 0 < exp.num_rows < full.num_rows and task.rows_out == exp.num_rows and task.rows_in == 1000 and ex_in.num_records() == 0
    assert joined.schema.names == ["value1", "avg(value2)", "count(*)"] and all(len(r[2]) == 3 for r in got)
    assert joined.column(0).to_pylist() == sorted(joined.column(0).to_pylist())


def test_aggregate_task_with_hidden_items_projects_them_away():
    batches = _batches()
    log = []
    sql = "select value1, min(id) as first from t group by value1 having count(*) > 9 and avg(value2) >= 40 and value1 < 'n'"
    err, task, ex_in, got, (keys, items, n_visible) = _run(
        batches, sql, filter_fn=_calls(log, "filter", O.filter_record), project_fn=_calls(log, "project", O.project_record))
    assert err is None and log == ["filter", "project"] and n_visible == 2 and [i.name for i in items[2:]] == ["__having_0", "__having_1"]
    full = _host_aggregate(batches, None, keys, items)
    exp = _as_projected(X.having(full, lambda r: r["__having_0"] > 9 and r["__having_1"] >= 40 and r["value1"] < "n").select([0, 1]))
    assert len(got) == 1 and batches_identical(got[0][1], exp), explain_diff(got[0][1], exp)
    assert 0 < exp.num_rows < full.num_rows and exp.schema.names == ["value1", "first"] and len(got[0][2]) == 2


def test_visible_items_that_share_a_name_keep_their_own_columns_behind_hidden_items():
    """the cut to the visible columns is positional: a projection by name alone would hand the first `x` out twice"""
    batches = _batches()
    seen = []

    def aggregate(records, aliases, keys, items):
        seen.append([i.name for i in items])
        return _host_aggregate(records, aliases, keys, items)

    sql = "select value1, count(*) as x, min(id) as x from t group by value1 having max(id) > 0"
    sel = parse_select(sql)
    keys, items, pred, n_visible = having_plan(sel)
    assert n_visible == 3 and [i.name for i in items] == ["value1", "x", "x", "__having_0"]
    ex_in = ExchangeOperator("operator_p0_exchange", ["operator_p1_producer"])
    ex_out = ExchangeOperator("operator_p1_exchange", ["operator_p2_producer"])
    for rid, b in enumerate(batches):
        ex_in.send_record(rid, b, [[] for _ in range(b.num_columns)])
    ex_in.producers_completed()
    task = AggregateOperatorTask(keys, items, 10_000, pred, n_visible)
    run = AggregateTaskBuilder(aggregate, O.filter_record, O.project_record).build(OperatorInstanceConfig(1, "operator_p1_producer", 5, task), [ex_in], ex_out)
    assert run() is None
    ex_out.producers_completed()
    got = ex_out.get_next_record("operator_p2_producer", 1)[1]
    assert seen == [["value1", "__visible_1", "__visible_2", "__having_0"]]      # the shared name never reaches the evaluator
    # the same SELECT without HAVING (every group has max(id) > 0), straight from the reference
    exp = _as_projected(_host_aggregate(batches, None, *aggregate_plan(parse_select("select value1, count(*) as x, min(id) as x from t group by value1"))))
    assert got.schema.names == ["value1", "x", "x"] and batches_identical(got, exp), explain_diff(got, exp)
    assert got.column(1).to_pylist() != got.column(2).to_pylist()
    # a visible column may already carry such a name: the stand-in moves on
    items2 = (A.AggItem(A.AggKind.COUNT_STAR, "__visible_1"), A.AggItem(A.AggKind.MIN, "x", -1, A.ident("id")),
              A.AggItem(A.AggKind.MAX, "x", -1, A.ident("id")), A.AggItem(A.AggKind.COUNT_STAR, "__having_0"))
    ex_in2 = ExchangeOperator("operator_p0_exchange", ["operator_p1_producer"])
    ex_out2 = ExchangeOperator("operator_p1_exchange", ["operator_p2_producer"])
    ex_in2.send_record(0, batches[0], [[] for _ in range(3)])
    ex_in2.producers_completed()
    task = AggregateOperatorTask((), items2, 10_000, A.binop(A.ident("__having_0"), A.BinaryOperator.Gt, A.number("0")), 3)
    run = AggregateTaskBuilder(_host_aggregate, O.filter_record, O.project_record).build(OperatorInstanceConfig(1, "operator_p1_producer", 5, task), [ex_in2], ex_out2)
    assert run() is None
    ex_out2.producers_completed()
    got = ex_out2.get_next_record("operator_p2_producer", 1)[1]
    ids = batches[0].column(0).to_pylist()
    assert got.schema.names == ["__visible_1", "x", "x"]
    assert [got.column(i).to_pylist() for i in range(3)] == [[len(ids)], [min(ids)], [max(ids)]]


def test_a_having_that_keeps_nothing_sends_one_empty_record_with_the_visible_schema():
    batches = simple_batches(100, 4, 33)
    err, task, _, got, _ = _run(batches, "select value1 from t group by value1 having count(*) > 1000000",
                                filter_fn=O.filter_record, project_fn=O.project_record)
    assert err is None and len(got) == 1 and got[0][1].num_rows == 0 and got[0][1].schema.names == ["value1"] and task.rows_out == 0


def test_a_failing_filter_keeps_the_inputs_unacked():
    batches = simple_batches(100, 4, 33)

    def boom(record, aliases, predicate):
        raise RuntimeError("filter failed")

    err, _, ex_in, got, _ = _run(batches, "select count(*) from t having count(*) > 1", filter_fn=boom)
    assert isinstance(err, RuntimeError) and ex_in.num_records() == len(batches) and got == []


def test_n_visible_must_name_some_of_the_items():
    task = AggregateOperatorTask((), (A.AggItem(A.AggKind.COUNT_STAR, "n"),), 50, None, 2)
    ex = ExchangeOperator("operator_p0_exchange", ["operator_p1_producer"])
    with pytest.raises(ValueError):
        AggregateTaskBuilder(_host_aggregate).build(OperatorInstanceConfig(1, "operator_p1_producer", 5, task), [ex], ex)


# ------------------------------------------------------------------------------------------------ avg_rn.h under the sanitizers
def rn_totals():
    """the totals the rounding can go wrong at, as (total, read as signed)"""
    both = [0, 1, 2**53, 2**53 + 1, 2**53 + 3, 2**95 + 1, 2**63 - 1, 2**52, 2**53 - 1, 2**54 + 2, 2**54 + 6, 2**64 - 2**10, 2**64 - 2**10 - 1,
            2**116 + 2**63, 2**116 + 2**64, 2**116 + 2**63 + 1, 2**117 - 1, 2**120 + 2**67, 2**120 + 2**67 + 1, 3 * 2**67, 2**126 + 2**73]
    unsigned = [2**64 - 1, 2**64,
                2**64 + 2**11,                    # a tie whose guard bit is in the low word: to even, 2^64
                2**64 + 2**11 + 1,                # sticky in the low word: up
                2**64 + 3 * 2**11,                # a tie on an odd mantissa: up
                (2**32 - 1) * (2**64 - 1),        # the largest total of 2^32 - 1 rows of UINT64_MAX
                2**64 - 2**10,                    # a mantissa of all ones that carries into the exponent: 2^64
                2**54 - 1, 2**128 - 1, 2**128 - 2**74, 2**128 - 2**74 - 1, 2**127, 2**127 + 2**74]
    signed = [-2**63, (2**32 - 1) * -2**63,       # ... of INT64_MIN
              (2**32 - 1) * (2**63 - 1), -2**127, 2**127 - 1, -(2**64 + 2**11), -(2**64 + 2**11 + 1)]
    rng = np.random.default_rng(5)
    for _ in range(3000):                         # random widths, with a run of ones or zeros below the mantissa
        p = int(rng.integers(1, 127))
        t = (1 << p) | int.from_bytes(rng.bytes(16), "little") % (1 << p)
        low = int(rng.integers(0, max(1, p - 52) + 1))
        both.append(t | ((1 << low) - 1) if rng.random() < 0.5 else t >> low << low)
    out = [(t, False) for t in both + unsigned] + [(s * t, True) for t in both for s in (1, -1) if t < 2**127] + [(t, True) for t in signed]
    return [(t, sg) for t, sg in out if (-2**127 <= t < 2**127 if sg else 0 <= t < 2**128)]


def test_the_table_holds_the_cases_by_name():
    assert float(2**64 + 2**11) == 2.0**64 and float(2**64 + 2**11 + 1) == 2.0**64 + 2.0**12 and float(2**64 - 2**10) == 2.0**64
    totals = rn_totals()
    for t in (0, 1, -1, 2**53, -2**53, 2**53 + 1, -(2**53 + 1), 2**53 + 3, -(2**53 + 3), 2**63 - 1, -2**63, 2**95 + 1, -(2**95 + 1)):
        assert (t, True) in totals
    for t in (2**64 - 1, 2**64, 2**64 + 2**11, 2**64 + 2**11 + 1, (2**32 - 1) * (2**64 - 1)):
        assert (t, False) in totals
    assert ((2**32 - 1) * -2**63, True) in totals and len(totals) > 9000


def test_avg_rounding_under_host_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler on PATH")
    import struct
    table = tmp_path / "totals.txt"
    totals = rn_totals()
    with open(table, "w") as f:
        for t, sg in totals:
            words = t % 2**128                                     # two's complement
            bits = struct.unpack("<Q", struct.pack("<d", float(t)))[0]
            f.write(f"{words >> 64:x} {words % 2**64:x} {int(sg)} {bits:x}\n")
    flags = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    # Whether this environment can build and run ANY sanitized program is settled first, on an empty one: only that may
    # skip.  Whatever happens to the program under test after that is a failure.
    probe_src, probe = tmp_path / "probe.cpp", str(tmp_path / "probe")
    probe_src.write_text("int main() { return 0; }\n")
    link = None
    for extra in (["-static-libasan", "-static-libubsan"], []):
        built = subprocess.run([cxx, *flags, *extra, str(probe_src), "-o", probe], capture_output=True, text=True)
        if built.returncode == 0:
            link = extra
            break
    if link is None:
        pytest.skip("the compiler cannot link an empty program with the sanitizers: " + (built.stderr.strip().splitlines() or ["?"])[-1])
    ran = subprocess.run([probe], capture_output=True, text=True)
    if ran.returncode != 0:
        pytest.skip("an empty sanitized program does not run here: " + (ran.stderr.strip().splitlines() or ["?"])[0])
    exe = str(tmp_path / "avg_main")
    build = subprocess.run([cxx, *flags, *link, os.path.join(ROOT, "tests", "avg_main.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe, str(table)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert run.stdout == f"{len(totals)} checks, 0 mismatches\n", run.stdout
