"""CPU: INNER JOIN without a GPU -- the host reference pinned to the oracle's filter_record over the left-major cross product
(the definition of the join) and to pyarrow's inner join as a multiset, the JOIN grammar and the
ON condition -> key pairs helper, and the join operator task over two in-process exchanges with the reference injected."""
import decimal

import numpy as np
import pyarrow as pa
import pytest

from chapterhouseqe_amd import sqlast as A
from chapterhouseqe_amd.operators import (ExchangeOperator, JoinOperatorTask, JoinTaskBuilder, OperatorInstanceConfig,
                                          build_default_operator_task_registry)
from chapterhouseqe_amd.sample_data import simple_batches
from chapterhouseqe_amd.sqlparse import Join, SqlParseError, TableFunc, join_plan, parse_select
from oracle import oracle as O
from tests import join_reference as J
from tests import sort_reference as R
from tests.helpers import batches_identical, explain_diff


# ------------------------------------------------------------------------------------------------ the reference
def _f32(bits):
    return pa.array(np.array(bits, dtype=np.uint32).view(np.float32))


def _f64(bits):
    return pa.array(np.array(bits, dtype=np.uint64).view(np.float64))


# -0 / +0, NaNs with two payloads (and a negative one), ordinary values
F32_POOL = [0x00000000, 0x80000000, 0x7FC00001, 0x7FC00002, 0xFFC00001, 0x3FC00000, 0xFF800000]
F64_POOL = [0x0000000000000000, 0x8000000000000000, 0x7FF8000000000001, 0x7FF8000000000002, 0xFFF8000000000001,
            0x3FF8000000000000, 0xFFF0000000000000]


def _pool(kind):
    if kind == "int8":
        return lambda ix: pa.array(np.array([-128, 127, 0, 1, -1], dtype=np.int8)[ix % 5])
    if kind == "int32":
        return lambda ix: pa.array(np.array([-2**31, 2**31 - 1, 0, 7, -7, 100], dtype=np.int32)[ix % 6])
    if kind == "int64":
        return lambda ix: pa.array(np.array([-2**63, 2**63 - 1, 0, 1 << 40, -(1 << 40)], dtype=np.int64)[ix % 5])
    if kind == "uint16":
        return lambda ix: pa.array(np.array([0, 65535, 1, 256, 32768], dtype=np.uint16)[ix % 5])
    if kind == "float32":
        return lambda ix: _f32([F32_POOL[i % len(F32_POOL)] for i in ix])
    if kind == "float64":
        return lambda ix: _f64([F64_POOL[i % len(F64_POOL)] for i in ix])
    if kind == "utf8":
        pool = ["", "a", "ab", "ab\x00", "b" * 40, "é"]
        return lambda ix: pa.array([pool[i % len(pool)] for i in ix], type=pa.utf8())
    if kind == "bool":
        return lambda ix: pa.array([bool(i % 2) for i in ix])
    if kind == "date32":
        return lambda ix: pa.array(np.array([-1, 0, 19000, 2**31 - 1], dtype=np.int32)[ix % 4]).view(pa.date32())
    if kind == "timestamp":
        return lambda ix: pa.array(np.array([-2**62, 0, 1_700_000_000_000_000, 5], dtype=np.int64)[ix % 4]).view(pa.timestamp("us", tz="UTC"))
    if kind == "decimal":
        pool = [decimal.Decimal("0.00"), decimal.Decimal("-0.01"), decimal.Decimal("123456789012345678.90"),
                decimal.Decimal("-123456789012345678.90"), decimal.Decimal("1.00")]
        return lambda ix: pa.array([pool[i % len(pool)] for i in ix], type=pa.decimal128(20, 2))
    raise ValueError(kind)


KEY_KINDS = ["int8", "int32", "int64", "uint16", "float32", "float64", "utf8", "bool", "date32", "timestamp", "decimal"]


def _with_nulls(arr, mask):
    """`arr` with the rows of `mask` null, its values buffer untouched (a float payload survives)"""
    if not mask.any():
        return arr
    return pa.Array.from_buffers(arr.type, len(arr), [pa.array(~mask).buffers()[1]] + arr.buffers()[1:], null_count=int(mask.sum()))


def _side(rng, n, kinds, row_name, null_rate=0.2):
    cols = [_with_nulls(_pool(k)(rng.integers(0, 1000, n)), rng.random(n) < null_rate) for k in kinds]
    names = ["k"] if len(kinds) == 1 else [f"k{i}" for i in range(len(kinds))]
    cols.append(pa.array(np.arange(n, dtype=np.int32)))
    cols.append(pa.array([f"{row_name}{i}" for i in range(n)], mask=rng.random(n) < 0.3))
    return pa.RecordBatch.from_arrays(cols, names=names + [row_name, "tag"])


def _on(names):
    e = None
    for n in names:
        eq = A.binop(A.compound("l", n), A.BinaryOperator.Eq, A.compound("r", n))
        e = eq if e is None else A.binop(e, A.BinaryOperator.And, eq)
    return e


def _check_against_the_oracle(left, right, names):
    lidx, ridx, exp = J.join(left, right, [(n, n) for n in names])
    cross = J.cross_product(left, right)
    aliases = [["l"]] * left.num_columns + [["r"]] * right.num_columns
    got = O.filter_record(cross, aliases, _on(names))
    assert batches_identical(got, exp), explain_diff(got, exp)
    assert lidx == sorted(lidx) and all(a < b for i, (a, b) in enumerate(zip(ridx, ridx[1:])) if lidx[i] == lidx[i + 1])
    return exp


@pytest.mark.parametrize("kind", KEY_KINDS)
def test_reference_is_the_filtered_cross_product(kind):
    rng = np.random.default_rng(KEY_KINDS.index(kind))
    left, right = _side(rng, 40, [kind], "lrow"), _side(rng, 50, [kind], "rrow")
    exp = _check_against_the_oracle(left, right, ["k"])
    assert 0 < exp.num_rows < 40 * 50
    assert exp.schema.names == ["k", "lrow", "tag", "k", "rrow", "tag"]
    assert exp.column(0).null_count == 0 and exp.column(3).null_count == 0       # a null key matches nothing


@pytest.mark.parametrize("kinds", [["int32", "utf8"], ["float32", "bool", "int8"], ["decimal", "timestamp"]])
def test_reference_with_several_keys(kinds):
    rng = np.random.default_rng(len(kinds) * 7 + len(kinds[0]))
    left, right = _side(rng, 40, kinds, "lrow", 0.1), _side(rng, 50, kinds, "rrow", 0.1)
    exp = _check_against_the_oracle(left, right, [f"k{i}" for i in range(len(kinds))])
    assert 0 < exp.num_rows < 40 * 50


def test_reference_float_equality_is_bitwise():
    left = pa.RecordBatch.from_arrays([_f32(F32_POOL), pa.array(np.arange(7, dtype=np.int32))], names=["k", "lrow"])
    right = pa.RecordBatch.from_arrays([_f32(F32_POOL[::-1] + F32_POOL[:3]), pa.array(np.arange(10, dtype=np.int32))], names=["k", "rrow"])
    lidx, ridx, exp = J.join(left, right, [("k", "k")])
    assert list(zip(lidx, ridx)) == [(0, 6), (0, 7), (1, 5), (1, 8), (2, 4), (2, 9), (3, 3), (4, 2), (5, 1), (6, 0)]
    _check_against_the_oracle(left, right, ["k"])


def test_reference_empty_sides_and_all_null_keys():
    rng = np.random.default_rng(3)
    left, right = _side(rng, 10, ["int32"], "lrow"), _side(rng, 10, ["int32"], "rrow")
    for l, r in ((left.slice(0, 0), right), (left, right.slice(0, 0)), (left.slice(0, 0), right.slice(0, 0))):
        lidx, ridx, exp = J.join(l, r, [("k", "k")])
        assert lidx == [] and exp.num_rows == 0 and exp.schema.names == ["k", "lrow", "tag", "k", "rrow", "tag"]
    nulls = pa.RecordBatch.from_arrays([pa.array([None] * 10, type=pa.int32()), left.column(1), left.column(2)], names=left.schema.names)
    assert J.join(nulls, right, [("k", "k")])[2].num_rows == 0
    _check_against_the_oracle(nulls, right, ["k"])


@pytest.mark.parametrize("kind", ["int8", "int32", "int64", "uint16", "utf8", "date32", "timestamp", "bool"])
def test_reference_agrees_with_arrow_as_a_multiset(kind):
    rng = np.random.default_rng(50 + KEY_KINDS.index(kind))
    left, right = _side(rng, 300, [kind], "lrow"), _side(rng, 200, [kind], "rrow")
    lidx, ridx, _ = J.join(left, right, [("k", "k")])
    lt = pa.Table.from_batches([left.select(["k", "lrow"]).rename_columns(["lk", "lrow"])])
    rt = pa.Table.from_batches([right.select(["k", "rrow"]).rename_columns(["rk", "rrow"])])
    arrow = lt.join(rt, keys="lk", right_keys="rk", join_type="inner", coalesce_keys=False, use_threads=False)
    pairs = sorted(zip(arrow.column("lrow").to_pylist(), arrow.column("rrow").to_pylist()))
    assert pairs == list(zip(lidx, ridx)) and len(pairs) > 100


# ------------------------------------------------------------------------------------------------ SQL
def test_parse_join_between_from_and_where():
    s = parse_select("select l.id, r.name from read_files('a/*.parquet') as l inner join read_files('b/*.parquet') as r "
                     "on l.id = r.id where l.id > 3 order by l.id limit 5")
    assert s.from_ == TableFunc("read_files", ("a/*.parquet",), "l")
    assert s.joins == (Join(TableFunc("read_files", ("b/*.parquet",), "r"),
                            A.binop(A.compound("l", "id"), A.BinaryOperator.Eq, A.compound("r", "id"))),)
    assert s.selection is not None and s.limit == 5 and len(s.order_by) == 1
    s2 = parse_select("select * from f('a') l join g('b') r on l.k = r.k")          # AS and INNER are optional
    assert s2.from_.alias == "l" and s2.joins[0].table == TableFunc("g", ("b",), "r") and s2.selection is None
    s3 = parse_select("SELECT * FROM f('a') JOIN g('b') ON a = b")                    # JOIN / ON never become an alias
    assert s3.from_.alias is None and s3.joins[0].table.alias is None
    assert parse_select("select a from read_files('x') t where a > 1").joins == ()
    assert join_plan(parse_select("select a from read_files('x') t")) is None


def test_select_positional_construction_still_works():
    s = parse_select("select id from read_files('x') where id > 1")
    assert s == type(s)(s.projection, s.from_, s.selection) == type(s)(s.projection, s.from_, s.selection, (), None, ())


def test_join_plan_normalises_both_operand_orders():
    lk, rk = A.compound("l", "id"), A.compound("r", "ident")
    for cond in ("l.id = r.ident", "r.ident = l.id", "(l.id = r.ident)", "((r.ident = l.id))"):
        assert join_plan(parse_select(f"select * from f('a') l join g('b') r on {cond}")) == ((lk, rk),), cond
    plan = join_plan(parse_select("select * from f('a') l join g('b') r on r.b = l.a and (l.c = r.d and r.e = l.f)"))
    assert plan == ((A.compound("l", "a"), A.compound("r", "b")), (A.compound("l", "c"), A.compound("r", "d")),
                    (A.compound("l", "f"), A.compound("r", "e")))
    assert J.from_plan(plan) == [("a", "b"), ("c", "d"), ("f", "e")]


@pytest.mark.parametrize("sql,names", [
    ("select * from f('a') l left join g('b') r on l.k = r.k", "only INNER JOIN"),
    ("select * from f('a') l left outer join g('b') r on l.k = r.k", "only INNER JOIN"),
    ("select * from f('a') l right join g('b') r on l.k = r.k", "only INNER JOIN"),
    ("select * from f('a') l full outer join g('b') r on l.k = r.k", "only INNER JOIN"),
    ("select * from f('a') l cross join g('b') r", "only INNER JOIN"),
    ("select * from f('a') left join g('b') r on l.k = r.k", "only INNER JOIN"),
    ("select * from f('a') l inner g('b') r on l.k = r.k", "JOIN"),
    ("select * from f('a') l join g('b') r where l.k = r.k", "ON"),
])
def test_parse_rejects_other_joins(sql, names):
    with pytest.raises(SqlParseError) as ei:
        parse_select(sql)
    assert names in str(ei.value)


@pytest.mark.parametrize("cond,term", [
    ("l.k < r.k", "l.k"),                          # not an equality
    ("l.k = r.k or l.a = r.a", "l.a"),             # not a conjunction
    ("l.k = l.a", "l.a"),                          # both columns of one side
    ("l.k = 5", "5"),                              # a literal
    ("k = r.k", "k"),                              # an unqualified column
    ("l.k = r.k and l.a + 1 = r.a", "l.a"),        # an expression
    ("l.k = x.k", "x.k"),                          # an alias of neither table
])
def test_join_plan_errors_name_the_term(cond, term):
    with pytest.raises(SqlParseError) as ei:
        join_plan(parse_select(f"select * from f('a') l join g('b') r on {cond}"))
    assert term in str(ei.value)


def test_join_plan_needs_two_distinct_aliases_and_one_join():
    for sql in ("select * from f('a') join g('b') r on l.k = r.k", "select * from f('a') l join g('b') on l.k = r.k",
                "select * from f('a') t join g('b') t on t.k = t.k",
                "select * from f('a') l join g('b') r on l.k = r.k join h('c') s on l.k = s.k"):
        with pytest.raises(SqlParseError):
            join_plan(parse_select(sql))


# ------------------------------------------------------------------------------------------------ the operator
def _host_join(left, left_aliases, right, right_aliases, keys):
    return J.join(left, right, J.from_plan(keys))[2]


def _dimension(n):
    rng = np.random.default_rng(5)
    return pa.RecordBatch.from_arrays([pa.array(rng.integers(0, 60, n).astype(np.int32)), pa.array([f"name{i}" for i in range(n)])],
                                      names=["id", "name"])


def _run_join(left, right, max_rows=10_000, join_fn=_host_join, out_cls=ExchangeOperator):
    keys = join_plan(parse_select("select * from read_files('a') l join read_files('b') r on r.id = l.id"))
    ex_l = ExchangeOperator("operator_l_exchange", ["operator_join_producer"])
    ex_r = ExchangeOperator("operator_r_exchange", ["operator_join_producer"])
    ex_out = out_cls("operator_join_exchange", ["operator_p2_producer"])
    for ex, batches, alias in ((ex_l, left, "l"), (ex_r, right, "r")):
        for rid, b in enumerate(batches):                    # both exchanges hand out record ids 0, 1, ...
            ex.send_record(rid, b, [[alias] for _ in range(b.num_columns)])
        ex.producers_completed()
    task = JoinOperatorTask(keys, max_rows)
    reg = build_default_operator_task_registry("/tmp")
    assert reg.find_task_builder(task) is reg.join_task and task.task_name() == "join"
    run = JoinTaskBuilder(join_fn).build(OperatorInstanceConfig(1, "operator_join_producer", 5, task), [ex_l, ex_r], ex_out)
    return run(), run.task, ex_l, ex_r, ex_out


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


def test_join_task_sends_the_pairs_in_left_major_order():
    left, right = simple_batches(100, 4, 33), [_dimension(150).slice(o, 50) for o in (0, 50, 100)]
    err, task, ex_l, ex_r, ex_out = _run_join(left, right, max_rows=40)
    assert err is None
    got = _drain(ex_out)
    exp = J.join(left, right, [("id", "id")])[2]
    assert exp.num_rows > 80 and exp.schema.names == ["id", "value1", "value2", "id", "name"]
    assert [r[0] for r in got] == list(range(len(got))) and len(got) == -(-exp.num_rows // 40)
    assert all(r[1].num_rows == 40 for r in got[:-1])
    assert all(r[2] == [["l"], ["l"], ["l"], ["r"], ["r"]] for r in got)      # left aliases, then right aliases
    joined = R.join([r[1] for r in got])
    assert batches_identical(joined, exp), explain_diff(joined, exp)
    assert ex_l.num_records() == 0 and ex_r.num_records() == 0
    assert task.rows_in == 250 and task.rows_out == exp.num_rows and task.records_sent == len(got)
    ids = joined.column(0).to_pylist()
    assert ids == sorted(ids)


def test_join_task_acks_only_after_the_sends():
    left, right = simple_batches(100, 4, 33), [_dimension(60)]
    seen = []
    holder = {}

    class Out(ExchangeOperator):
        def send_record(self, record_id, record, table_aliases):
            seen.append((holder["l"].num_records(), holder["r"].num_records()))   # every input still held when the output goes out
            super().send_record(record_id, record, table_aliases)

    keys = join_plan(parse_select("select * from f('a') l join f('b') r on l.id = r.id"))
    ex_l = ExchangeOperator("operator_l_exchange", ["operator_join_producer"])
    ex_r = ExchangeOperator("operator_r_exchange", ["operator_join_producer"])
    holder["l"], holder["r"] = ex_l, ex_r
    ex_out = Out("operator_join_exchange", ["operator_p2_producer"])
    for ex, batches in ((ex_l, left), (ex_r, right)):
        for rid, b in enumerate(batches):
            ex.send_record(rid, b, [[] for _ in range(b.num_columns)])
        ex.producers_completed()
    run = JoinTaskBuilder(_host_join).build(OperatorInstanceConfig(1, "operator_join_producer", 5, JoinOperatorTask(keys, 25)), [ex_l, ex_r], ex_out)
    assert run() is None
    assert len(seen) > 1 and all(s == (len(left), 1) for s in seen)
    assert ex_l.num_records() == 0 and ex_r.num_records() == 0


@pytest.mark.parametrize("empty", ["left", "right", "both"])
def test_join_task_with_an_empty_side_sends_nothing(empty):
    left = [] if empty in ("left", "both") else simple_batches(100, 4, 33)
    right = [] if empty in ("right", "both") else [_dimension(60)]
    err, task, ex_l, ex_r, ex_out = _run_join(left, right)
    assert err is None
    assert _drain(ex_out) == [] and task.records_sent == 0
    assert ex_l.num_records() == 0 and ex_r.num_records() == 0          # what did come in is acked


def test_join_task_without_matches_sends_one_empty_record():
    left = simple_batches(100, 4, 33)
    right = [pa.RecordBatch.from_arrays([pa.array([-5, -6], type=pa.int32()), pa.array(["x", "y"])], names=["id", "name"])]
    err, task, _, _, ex_out = _run_join(left, right)
    assert err is None
    got = _drain(ex_out)
    assert len(got) == 1 and got[0][1].num_rows == 0 and got[0][1].schema.names == ["id", "value1", "value2", "id", "name"]


def test_a_failing_join_keeps_the_inputs_unacked():
    left, right = simple_batches(100, 4, 33), [_dimension(60)]

    def boom(*args):
        raise RuntimeError("join failed")

    err, task, ex_l, ex_r, ex_out = _run_join(left, right, join_fn=boom)
    assert isinstance(err, RuntimeError)
    assert ex_l.num_records() == len(left) and ex_r.num_records() == 1 and ex_out.num_records() == 0


def test_join_task_takes_two_inbound_exchanges():
    keys = join_plan(parse_select("select * from f('a') l join f('b') r on l.id = r.id"))
    ex = ExchangeOperator("operator_l_exchange", ["operator_join_producer"])
    with pytest.raises(ValueError):
        JoinTaskBuilder(_host_join).build(OperatorInstanceConfig(1, "operator_join_producer", 5, JoinOperatorTask(keys)), [ex], None)
