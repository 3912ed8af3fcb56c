"""CPU: window functions without a GPU -- the host reference of tests/window_reference.py pinned to sqlite3 (standard library)
where the two share semantics and to identities where they do not (bit-pattern partitions, the frames against GROUP BY),
the OVER grammar and `window_plan`, the unchanged parse of statements without OVER, and the window operator task over the
in-process exchange with the reference injected."""
import math
import sqlite3

import numpy as np
import pyarrow as pa
import pytest

from chapterhouseqe_amd import sqlast as A
from chapterhouseqe_amd.operators import (ExchangeOperator, OperatorInstanceConfig, WindowOperatorTask, WindowTaskBuilder,
                                          build_default_operator_task_registry)
from chapterhouseqe_amd.sample_data import simple_batches
from chapterhouseqe_amd.sqlparse import (Select, SqlParseError, TableFunc, aggregate_plan, is_aggregate_call, parse_select, window_plan)
from tests import aggregate_reference as G
from tests import sort_reference as R
from tests import window_reference as W
from tests.helpers import batches_identical, explain_diff


# ------------------------------------------------------------------------------------------------ the reference against sqlite
_FRAME_SQL = {"rows": "rows between unbounded preceding and current row", "range": "range between unbounded preceding and current row",
              "partition": "rows between unbounded preceding and unbounded following"}


def _sqlite_window(batch, partition_by, order_by, items):
    """the rows of `batch` in input order with one more column per item, by sqlite.  sqlite does not promise stable ties:
    where the result depends on them (row_number, lag / lead, the ROWS frame) the row id is the last ORDER BY term."""
    con = sqlite3.connect(":memory:")
    names = batch.schema.names
    con.execute(f"create table t (rid integer, {', '.join(names)})")
    rows = zip(*[batch.column(i).to_pylist() for i in range(batch.num_columns)])
    con.executemany(f"insert into t values ({', '.join('?' * (len(names) + 1))})", [(r,) + tuple(v) for r, v in enumerate(rows)])

    def over(stable, frame=""):
        keys = [f"{k} {'desc' if d else 'asc'} nulls {'first' if nf else 'last'}" for k, d, nf in order_by] + (["rid"] if stable else [])
        part = f"partition by {', '.join(partition_by)} " if partition_by else ""
        order = f"order by {', '.join(keys)} " if keys else ""
        return f"over ({part}{order}{frame})"

    cols = []
    for kind, name, col, frame, offset in items:
        if kind == "row_number":
            cols.append(f"row_number() {over(True)}")
        elif kind in ("rank", "dense_rank"):
            cols.append(f"{kind}() {over(False)}")
        elif kind in ("lag", "lead"):
            cols.append(f"{kind}({col}, {offset}) {over(True)}")
        else:
            fn = "count(*)" if kind == "count_star" else f"{kind}({col})"
            cols.append(f"{fn} {over(frame == 'rows', _FRAME_SQL[frame])}")
    got = con.execute(f"select {', '.join(cols)} from t order by rid").fetchall()
    con.close()
    return [list(c) for c in zip(*got)] if got else [[] for _ in items]


def _sqlite_batch(rng, n):
    strs = ["".join(chr(97 + c) for c in rng.integers(0, 3, rng.integers(0, 4))) for _ in range(n)]
    return pa.RecordBatch.from_arrays([
        pa.array(rng.integers(-4, 4, n), type=pa.int64(), mask=rng.random(n) < 0.1),
        pa.array(strs, mask=rng.random(n) < 0.1),
        pa.array(np.round(rng.standard_normal(n), 1) + 0.25, mask=rng.random(n) < 0.1),
        pa.array(rng.integers(-2**50, 2**50, n), type=pa.int64(), mask=rng.random(n) < 0.3),
        pa.array(rng.standard_normal(n) * 1e3, mask=rng.random(n) < 0.3),
        pa.array(["%c%c" % (97 + a, 97 + b) for a, b in rng.integers(0, 26, (n, 2))], mask=rng.random(n) < 0.2)],
        names=["k", "s", "f", "v", "w", "t"])


def _all_items(order_cols):
    items = [("row_number", "rn", None, "partition", 0), ("rank", "rk", None, "partition", 0), ("dense_rank", "dr", None, "partition", 0),
             ("lag", "lag_v", "v", "partition", 1), ("lead", "lead_t", "t", "partition", 2), ("lag", "lag0", "w", "partition", 0),
             ("lead", "lead_far", "v", "partition", 10_000)]
    for frame in W.FRAMES:
        items += [("count_star", f"n_{frame}", None, frame, 0), ("count", f"c_{frame}", "v", frame, 0), ("sum", f"sv_{frame}", "v", frame, 0),
                  ("sum", f"sw_{frame}", "w", frame, 0), ("min", f"lo_{frame}", "w", frame, 0), ("max", f"hi_{frame}", "v", frame, 0)]
    return items


@pytest.mark.parametrize("partition_by,order_by", [
    (["k"], [("f", False, False)]),
    (["s"], [("v", True, True)]),
    (["k", "s"], [("f", True, False), ("v", False, True)]),
    ([], [("s", False, True)]),
    (["f"], []),
    ([], []),
])
def test_reference_agrees_with_sqlite(partition_by, order_by):
    rng = np.random.default_rng(17)
    b = _sqlite_batch(rng, 700)
    # sqlite turns NaN into NULL, treats -0 = +0 and sums integers in 64 bits: none of that may be in these inputs
    for c in ("f", "w"):
        x = b.column(b.schema.get_field_index(c)).drop_null().to_numpy()
        assert np.isfinite(x).all() and not (np.signbit(x) & (x == 0)).any()
    assert sum(abs(v) for v in b.column(3).drop_null().to_pylist()) < 2**63
    items = _all_items(order_by)
    exp, bounds = W.window(b, partition_by, order_by, items)
    lite = _sqlite_window(b, partition_by, order_by, items)
    assert exp.num_rows == b.num_rows and exp.schema.names[:6] == b.schema.names
    for i, (kind, name, col, frame, offset) in enumerate(items):
        ci = b.num_columns + i
        ours = exp.column(ci).to_pylist()
        if ci in bounds:   # a float sum: sqlite adds in binary64 in its own order
            ns, mags = bounds[ci]
            for r, (x, y) in enumerate(zip(ours, lite[i])):
                assert (x is None) == (y is None), (name, r)
                assert x is None or abs(x - y) <= float(ns[r]) * 2.0**-52 * float(mags[r]), (name, r, x, y)
        else:
            assert ours == lite[i], (name, [(r, x, y) for r, (x, y) in enumerate(zip(ours, lite[i])) if x != y][:5])
    assert len(bounds) == 3


# ------------------------------------------------------------------------------------------------ identities
def _edge_batch(rng, n):
    """what sqlite cannot check: -0 / +0, NaN payloads, infinities"""
    pats = np.array([0x0000000000000000, 0x8000000000000000, 0x7FF8000000000001, 0x7FF8000000000002, 0x3FF0000000000000], dtype=np.uint64)
    return pa.RecordBatch.from_arrays([
        pa.array(pats[rng.integers(0, len(pats), n)].view(np.float64), mask=rng.random(n) < 0.1),
        pa.array(rng.integers(0, 5, n).astype(np.int16), mask=rng.random(n) < 0.1),
        pa.array(rng.choice([1.5, -2.25, np.inf, -np.inf, np.nan, 0.0], n, p=[0.45, 0.45, 0.02, 0.02, 0.02, 0.04]), mask=rng.random(n) < 0.2),
        pa.array(rng.integers(-100, 100, n).astype(np.int32), mask=rng.random(n) < 0.2),
        pa.array((rng.random(n) * 8).astype(np.float32))], names=["f", "k", "x", "v", "y"])


def test_partition_frame_is_group_by_broadcast_to_the_rows():
    rng = np.random.default_rng(3)
    b = _edge_batch(rng, 2000)
    for keys in (["f"], ["k"], ["k", "f"], []):
        items = [("count_star", "n", None, "partition", 0), ("count", "c", "x", "partition", 0), ("sum", "sx", "x", "partition", 0),
                 ("sum", "sv", "v", "partition", 0), ("min", "lo", "x", "partition", 0), ("max", "hi", "y", "partition", 0)]
        exp, _ = W.window(b, keys, [("v", False, False)], items)
        grouped, _ = G.aggregate(b, keys, [(kind, name, col) for kind, name, col, _, _ in items])
        for g, rows in enumerate(G.group_rows(b, keys)):
            for i in range(len(items)):
                want = grouped.column(i).slice(g, 1)
                got = exp.column(b.num_columns + i).take(pa.array(rows, type=pa.int64()))
                for r in range(len(rows)):
                    assert _same(got[r], want[0]), (keys, items[i][1], g)


def _same(a, b):
    if not a.is_valid or not b.is_valid:
        return a.is_valid == b.is_valid
    x, y = a.as_py(), b.as_py()
    if isinstance(x, float):
        return np.float64(x).view(np.uint64) == np.float64(y).view(np.uint64) or (math.isnan(x) and math.isnan(y))
    return x == y


def test_row_number_is_a_permutation_and_the_last_row_under_rows_is_the_partition():
    rng = np.random.default_rng(4)
    b = _edge_batch(rng, 1500)
    items = [("row_number", "rn", None, "partition", 0), ("sum", "rows", "v", "rows", 0), ("sum", "all", "v", "partition", 0),
             ("sum", "frows", "x", "rows", 0), ("sum", "fall", "x", "partition", 0), ("count_star", "n", None, "partition", 0),
             ("min", "lo_rows", "y", "rows", 0), ("min", "lo_all", "y", "partition", 0)]
    exp, _ = W.window(b, ["k"], [("y", True, False)], items)
    nc = b.num_columns
    for rows in G.group_rows(b, ["k"]):
        part = exp.take(pa.array(rows, type=pa.int64()))
        rn = part.column(nc).to_pylist()
        assert sorted(rn) == list(range(1, len(rows) + 1))
        last = rn.index(len(rows))
        assert part.column(nc + 5).to_pylist() == [len(rows)] * len(rows)
        for a, c in ((nc + 1, nc + 2), (nc + 3, nc + 4), (nc + 6, nc + 7)):
            assert _same(part.column(a)[last], part.column(c)[last])


def test_zero_signs_and_nan_payloads_are_partitions_and_peers_of_their_own():
    bits = np.array([0x00000000, 0x80000000, 0x7FC00001, 0x7FC00002, 0x00000000, 0x7FC00001, 0x80000000], dtype=np.uint32)
    b = pa.RecordBatch.from_arrays([pa.array(bits.view(np.float32)), pa.array(np.arange(7, dtype=np.int32))], names=["f", "row"])
    items = [("count_star", "n", None, "partition", 0), ("row_number", "rn", None, "partition", 0)]
    exp, _ = W.window(b, ["f"], [], items)
    assert exp.column(2).to_pylist() == [2, 2, 2, 1, 2, 2, 2] and exp.column(3).to_pylist() == [1, 1, 1, 1, 2, 2, 2]
    # as order keys (totalOrder: -0 < +0 < NaN(1) < NaN(2)): four peer groups
    items = [("rank", "rk", None, "partition", 0), ("dense_rank", "dr", None, "partition", 0), ("count_star", "n", None, "range", 0)]
    exp, _ = W.window(b, [], [("f", False, False)], items)
    assert exp.column(2).to_pylist() == [3, 1, 5, 7, 3, 5, 1]
    assert exp.column(3).to_pylist() == [2, 1, 3, 4, 2, 3, 1]
    assert exp.column(4).to_pylist() == [4, 2, 6, 7, 4, 6, 2]


def test_integer_overflow_is_decided_per_frame():
    b = pa.RecordBatch.from_arrays([pa.array([2**63 - 1, 1, -5], type=pa.int64()), pa.array([0, 1, 2], type=pa.int32())], names=["v", "o"])
    exp, _ = W.window(b, [], [("o", False, False)], [("sum", "s", "v", "partition", 0)])
    assert exp.column(2).to_pylist() == [2**63 - 5] * 3
    with pytest.raises(G.SumOverflow):
        W.window(b, [], [("o", False, False)], [("sum", "s", "v", "rows", 0)])
    exp, _ = W.window(b, [], [("o", True, False)], [("sum", "s", "v", "rows", 0)])   # -5, 1, then the maximum: never outside
    assert exp.column(2).to_pylist() == [2**63 - 5, -4, -5]


def test_empty_input_keeps_the_schema():
    b = _edge_batch(np.random.default_rng(1), 5).slice(0, 0)
    exp, bounds = W.window(b, ["k"], [("v", False, False)], _items_for_edge())
    assert exp.num_rows == 0 and exp.schema.names[5:] == [it[1] for it in _items_for_edge()]
    assert exp.schema.field("lag_x").nullable and not exp.schema.field("rn").nullable and exp.schema.field("lag_x").type == pa.float64()


def _items_for_edge():
    return [("row_number", "rn", None, "partition", 0), ("lag", "lag_x", "x", "partition", 1), ("sum", "s", "x", "rows", 0),
            ("max", "hi", "v", "range", 0)]


# ------------------------------------------------------------------------------------------------ the grammar
def _calls(sql):
    return [f.expr for f in parse_select(sql).projection]


def test_over_clause_and_its_defaults():
    e, = _calls("select row_number() over (partition by a, t.b order by c desc nulls last, d) from t")
    assert isinstance(e, A.Function) and isinstance(e, A.UnsupportedExpr) and e.debug == "Function(row_number)" and e.args == ()
    assert e.over == A.WindowSpec((A.ident("a"), A.compound("t", "b")),
                                  (A.OrderByExpr(A.ident("c"), False, False), A.OrderByExpr(A.ident("d"), None, None)),
                                  A.WindowFrame.RANGE_TO_CURRENT)
    frames = {"": A.WindowFrame.PARTITION,
              "order by c": A.WindowFrame.RANGE_TO_CURRENT,
              "order by c rows between unbounded preceding and current row": A.WindowFrame.ROWS_TO_CURRENT,
              "order by c RANGE BETWEEN UNBOUNDED PRECEDING AND CURRENT ROW": A.WindowFrame.RANGE_TO_CURRENT,
              "order by c rows between unbounded preceding and unbounded following": A.WindowFrame.PARTITION,
              "order by c range between unbounded preceding and unbounded following": A.WindowFrame.PARTITION,
              "partition by a rows between unbounded preceding and current row": A.WindowFrame.ROWS_TO_CURRENT,
              "partition by a": A.WindowFrame.PARTITION}
    for text, frame in frames.items():
        e, = _calls(f"select sum(v) OVER ({text}) from t")
        assert e.over.frame == frame and not is_aggregate_call(e), text
    assert is_aggregate_call(_calls("select sum(v) from t")[0])
    assert _calls("select sum(v) from t")[0].over is None


def test_window_plan():
    sel = parse_select("select id, row_number() over (partition by b order by v desc) as rn, sum(v) over (partition by b order by v desc "
                       "rows between unbounded preceding and current row), Lag(s) over (partition by b order by v desc), "
                       "lead(s, 3) over (partition by b order by v desc) nxt, count(*) over (partition by b order by v desc), "
                       "max(v) over (partition by b order by v desc range between unbounded preceding and unbounded following) top "
                       "from t where id > 3")
    partition_by, order_by, items, projection = window_plan(sel)
    assert partition_by == (A.ident("b"),) and order_by == (A.OrderByExpr(A.ident("v"), False, None),)
    K, F = A.WindowKind, A.WindowFrame
    assert items == (A.WindowItem(K.ROW_NUMBER, "rn"),
                     A.WindowItem(K.SUM, "sum(v)", A.ident("v"), F.ROWS_TO_CURRENT),
                     A.WindowItem(K.LAG, "lag(s)", A.ident("s"), F.PARTITION, 1),
                     A.WindowItem(K.LEAD, "nxt", A.ident("s"), F.PARTITION, 3),
                     A.WindowItem(K.COUNT_STAR, "count(*)", None, F.RANGE_TO_CURRENT),
                     A.WindowItem(K.MAX, "top", A.ident("v"), F.PARTITION))
    assert projection == (A.UnnamedExpr(A.ident("id")), A.ExprWithAlias(A.ident("rn"), A.Ident("rn")), A.UnnamedExpr(A.ident("sum(v)")),
                          A.UnnamedExpr(A.ident("lag(s)")), A.ExprWithAlias(A.ident("nxt"), A.Ident("nxt")),
                          A.UnnamedExpr(A.ident("count(*)")), A.ExprWithAlias(A.ident("top"), A.Ident("top")))
    assert aggregate_plan(sel) is None
    assert window_plan(parse_select("select a, sum(v) from t group by a")) is None
    assert window_plan(parse_select("select * from t")) is None
    p, o, it, proj = window_plan(parse_select("select *, rank() over () from t"))
    assert p == () and o == () and it == (A.WindowItem(K.RANK, "rank()"),) and proj[0] == A.Wildcard()


@pytest.mark.parametrize("sql", [
    "select sum(v) over (order by c rows between 1 preceding and current row) from t",
    "select sum(v) over (order by c rows unbounded preceding) from t",
    "select sum(v) over (order by c rows between current row and unbounded following) from t",
    "select sum(v) over (order by c groups between unbounded preceding and current row) from t",
    "select sum(v) over (order by c range between unbounded preceding and 1 following) from t",
    "select sum(v) over (partition a) from t",
    "select sum(v) over (order c) from t",
    "select sum(v) over (partition by a from t",
    "select sum(v) over w from t",
])
def test_over_clause_errors(sql):
    with pytest.raises(SqlParseError):
        parse_select(sql)


@pytest.mark.parametrize("sql", [
    "select rank() over (partition by a), sum(v) over (partition by b) from t",            # two window specifications
    "select rank() over (order by a), sum(v) over (order by a desc) from t",
    "select a, rank() over (order by a), sum(v) from t",                                   # a plain aggregate beside it
    "select a, rank() over (order by a) from t group by a",
    "select 1 + rank() over (order by a) from t",                                          # not a whole SELECT item
    "select first_value(a) over (order by a) from t",                                      # out of scope
    "select ntile(4) over (order by a) from t",
    "select avg(a) over (order by a) from t",
    "select rank(a) over (order by a) from t",
    "select lag() over (order by a) from t",
    "select lag(a, 1, 0) over (order by a) from t",                                        # no default-value argument
    "select lag(a, b) over (order by a) from t",
    "select lag(a, -1) over (order by a) from t",
    "select lag(a, 1.5) over (order by a) from t",
    "select sum(*) over (order by a) from t",
    "select sum(a, b) over (order by a) from t",
    "select count(distinct a) over (order by a) from t",
    "select sum(a) over (order by a), sum(a) over (order by a rows between unbounded preceding and current row) from t",   # one name twice
])
def test_window_plan_errors(sql):
    with pytest.raises(SqlParseError):
        window_plan(parse_select(sql))


def test_statements_without_over_parse_as_before():
    i, c, num = A.ident, A.compound, A.number
    Op = A.BinaryOperator
    t = TableFunc("read_files", ("simple/*.parquet",), None)
    assert parse_select("select * from read_files('simple/*.parquet') where id > 25") == Select(
        (A.Wildcard(),), t, A.BinaryOp(i("id"), Op.Gt, num("25")))
    assert parse_select("select id, value2 + 1 as v from read_files('simple/*.parquet') order by value2 desc nulls last, id limit 10") == Select(
        (A.UnnamedExpr(i("id")), A.ExprWithAlias(A.BinaryOp(i("value2"), Op.Plus, num("1")), A.Ident("v"))), t, None,
        (A.OrderByExpr(i("value2"), False, False), A.OrderByExpr(i("id"), None, None)), 10)
    assert parse_select("select value1, count(*), sum(value2) total from t where id > 100 group by value1") == Select(
        (A.UnnamedExpr(i("value1")), A.UnnamedExpr(A.Function("Function(count)", "count", (), True)),
         A.ExprWithAlias(A.Function("Function(sum)", "sum", (i("value2"),), False), A.Ident("total"))),
        TableFunc("t", (), None), A.BinaryOp(i("id"), Op.Gt, num("100")), (), None, (i("value1"),))
    s = parse_select("select l.id, r.value2 from read_files('a') l inner join read_files('b') as r on l.id = r.id and (l.k = r.k)")
    assert s.projection == (A.UnnamedExpr(c("l", "id")), A.UnnamedExpr(c("r", "value2")))
    assert s.from_ == TableFunc("read_files", ("a",), "l") and s.joins[0].table == TableFunc("read_files", ("b",), "r")
    assert s.joins[0].on == A.BinaryOp(A.BinaryOp(c("l", "id"), Op.Eq, c("r", "id")), Op.And,
                                       A.Nested(A.BinaryOp(c("l", "k"), Op.Eq, c("r", "k"))))
    f = parse_select("select abs(a) over_ from t").projection[0]                      # a word that merely begins like OVER
    assert f == A.ExprWithAlias(A.Function("Function(abs)", "abs", (i("a"),), False), A.Ident("over_"))
    assert A.Function("Function(abs)", "abs", (i("a"),)).over is None
    assert repr(parse_select("select -abs(a) from t").projection[0].expr) == \
        "UnsupportedExpr(debug=\"UnaryOp { op: Minus, expr: UnsupportedExpr(debug='Function(abs)') }\")"


# ------------------------------------------------------------------------------------------------ the operator
def _host_window(records, aliases, partition_by, order_by, items):
    rp, ro, ri = W.from_plan(partition_by, order_by, items)
    return W.window_batches(records, rp, ro, ri)[0]


def _host_project(fields, rec, aliases):
    """identifiers and aliases only: what `window_plan` leaves of the SELECT list in these tests"""
    arrays, out = [], []
    for f in fields:
        assert isinstance(f, (A.UnnamedExpr, A.ExprWithAlias)) and isinstance(f.expr, A.Identifier)
        c = rec.schema.get_field_index(f.expr.ident.value)
        arrays.append(rec.column(c))
        out.append(rec.schema.field(c).with_name(f.alias.value if isinstance(f, A.ExprWithAlias) else f.expr.ident.value))
    return pa.RecordBatch.from_arrays(arrays, schema=pa.schema(out))


def _run_window(batches, sql, max_rows=10_000, window_fn=_host_window, out_cls=ExchangeOperator):
    partition_by, order_by, items, projection = window_plan(parse_select(sql))
    ex_in = ExchangeOperator("operator_p0_exchange", ["operator_p1_producer"])
    ex_out = out_cls("operator_p1_exchange", ["operator_p2_producer"])
    for rid, b in enumerate(batches):
        ex_in.send_record(rid, b, [[] for _ in range(b.num_columns)])
    ex_in.producers_completed()
    task = WindowOperatorTask(partition_by, order_by, items, projection, max_rows)
    reg = build_default_operator_task_registry("/tmp")
    assert reg.find_task_builder(task) is reg.window_task
    run = WindowTaskBuilder(window_fn, _host_project).build(OperatorInstanceConfig(1, "operator_p1_producer", 5, task), [ex_in], ex_out)
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


SQL = ("select id, row_number() over (partition by value1 order by value2 desc) as rn, value1, "
       "sum(value2) over (partition by value1 order by value2 desc rows between unbounded preceding and current row) running, "
       "lag(id, 2) over (partition by value1 order by value2 desc) from t")


def test_window_task_sends_every_row_in_input_order():
    batches = simple_batches(1000, 4, 33)
    err, task, ex_in, ex_out = _run_window(batches, SQL, max_rows=100)
    assert err is None
    got = _drain(ex_out)
    joined_in = R.join(batches)
    full, _ = W.window(joined_in, ["value1"], [("value2", True, True)],
                       [("row_number", "rn", None, "partition", 0), ("sum", "running", "value2", "rows", 0), ("lag", "lag(id, 2)", "id", "partition", 2)])
    exp = full.select(["id", "rn", "value1", "running", "lag(id, 2)"])
    assert [r[0] for r in got] == list(range(10)) and all(len(r[2]) == 5 for r in got)
    joined = R.join([r[1] for r in got])
    assert batches_identical(joined, exp), explain_diff(joined, exp)
    assert joined.column(0).to_pylist() == joined_in.column(0).to_pylist()           # input order
    assert ex_in.num_records() == 0 and task.rows_in == 1000 and task.rows_out == 1000 and task.records_sent == 10


def test_window_task_without_input_sends_nothing_and_an_error_requeues():
    err, task, _, ex_out = _run_window([], SQL)
    assert err is None and _drain(ex_out) == [] and task.records_sent == 0

    def boom(*args):
        raise RuntimeError("no window today")

    batches = simple_batches(100, 4, 33)
    err, task, ex_in, ex_out = _run_window(batches, SQL, window_fn=boom)
    assert isinstance(err, RuntimeError)
    assert ex_in.num_records() == len(batches) and ex_out.num_records() == 0


def test_window_task_config_errors():
    item = A.WindowItem(A.WindowKind.RANK, "r")
    proj = (A.UnnamedExpr(A.ident("r")),)
    for task in (WindowOperatorTask((), (), (), proj), WindowOperatorTask((), (), (item,), ()), WindowOperatorTask((), (), (item,), proj, 0)):
        with pytest.raises(ValueError):
            WindowTaskBuilder().build(OperatorInstanceConfig(1, "operator_p1_producer", 5, task), [], None)
