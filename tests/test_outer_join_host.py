"""CPU: the join kinds without a GPU -- the host reference of tests/outer_join_reference.py pinned to identities over the INNER
reference and to pyarrow's joins as row multisets, float keys by bits, the join operator task with the reference injected
for every kind, and the parts of the interface that need no device."""
import collections

import numpy as np
import pyarrow as pa
import pytest

from chapterhouseqe_amd import _lib, record_utils
from chapterhouseqe_amd.operators import ExchangeOperator, JoinOperatorTask, JoinTaskBuilder, OperatorInstanceConfig
from chapterhouseqe_amd.sample_data import simple_batches
from chapterhouseqe_amd.sqlparse import join_plan, parse_select
from tests import join_reference as J
from tests import outer_join_reference as OJ
from tests import sort_reference as R
from tests.helpers import batches_identical, explain_diff
from tests.test_join_host import F32_POOL, _f32, _side

KEYSETS = [["int32"], ["int32", "utf8", "bool"]]


def _sides(kinds, seed=0):
    rng = np.random.default_rng(seed + len(kinds))
    left, right = _side(rng, 300, kinds, "lrow", 0.15), _side(rng, 200, kinds, "rrow", 0.15)
    names = ["k"] if len(kinds) == 1 else [f"k{i}" for i in range(len(kinds))]
    return left, right, [(n, n) for n in names]


def _rows(lidx, ridx):
    return list(zip(lidx, ridx))


# ------------------------------------------------------------------------------------------------ identities
@pytest.mark.parametrize("kinds", KEYSETS)
def test_inner_is_the_inner_reference(kinds):
    left, right, keys = _sides(kinds)
    lidx, ridx, exp = J.join(left, right, keys)
    got = OJ.join(left, right, keys, "inner")
    assert (got[0], got[1]) == (lidx, ridx) and len(lidx) > 50
    assert batches_identical(got[2], exp), explain_diff(got[2], exp)


@pytest.mark.parametrize("kinds", KEYSETS)
def test_left_is_inner_merged_with_the_padded_anti_rows(kinds):
    left, right, keys = _sides(kinds)
    inner = _rows(*J.join_indices(left, right, keys))
    anti = OJ.join_indices(left, right, keys, "anti")[0]
    assert inner and anti
    merged = sorted(inner + [(l, None) for l in anti], key=lambda p: (p[0], -1 if p[1] is None else p[1]))
    assert _rows(*OJ.join_indices(left, right, keys, "left")) == merged
    exp = OJ.join(left, right, keys, "left")[2]
    assert all(exp.schema.field(i).nullable for i in range(left.num_columns, exp.num_columns))
    pad = [i for i, r in enumerate(OJ.join_indices(left, right, keys, "left")[1]) if r is None]
    for c in range(left.num_columns, exp.num_columns):
        assert all(not exp.column(c)[i].is_valid for i in pad)


@pytest.mark.parametrize("kinds", KEYSETS)
def test_semi_and_anti_partition_the_left_rows(kinds):
    left, right, keys = _sides(kinds)
    semi, none_s = OJ.join_indices(left, right, keys, "semi")
    anti, none_a = OJ.join_indices(left, right, keys, "anti")
    assert none_s is None and none_a is None and semi and anti
    assert sorted(semi + anti) == list(range(left.num_rows)) and not set(semi) & set(anti)
    assert semi == sorted(set(J.join_indices(left, right, keys)[0]))
    null_rows = [i for i, k in enumerate(J._row_keys(left, [lk for lk, _ in keys])) if k is None]
    assert null_rows and set(null_rows) <= set(anti)                      # NOT EXISTS: a null key has no match
    exp = OJ.join(left, right, keys, "semi")[2]
    assert exp.schema == left.schema and batches_identical(exp, left.take(pa.array(semi)))


@pytest.mark.parametrize("kinds", KEYSETS)
def test_full_is_left_followed_by_the_unmatched_right_rows(kinds):
    left, right, keys = _sides(kinds)
    l_l, l_r = OJ.join_indices(left, right, keys, "left")
    f_l, f_r = OJ.join_indices(left, right, keys, "full")
    matched = set(J.join_indices(left, right, keys)[1])
    tail = [r for r in range(right.num_rows) if r not in matched]
    assert tail and f_l == l_l + [None] * len(tail) and f_r == l_r + tail
    exp = OJ.join(left, right, keys, "full")[2]
    assert all(f.nullable for f in exp.schema) and exp.num_rows == len(l_l) + len(tail)


@pytest.mark.parametrize("kinds", KEYSETS)
def test_right_is_left_with_the_sides_exchanged(kinds):
    left, right, keys = _sides(kinds)
    swapped = OJ.join(right, left, [(rk, lk) for lk, rk in keys], "left")
    lidx, ridx, exp = OJ.join(left, right, keys, "right")
    assert (lidx, ridx) == (swapped[1], swapped[0]) and None in lidx
    nr = right.num_columns
    back = swapped[2].select(list(range(nr, nr + left.num_columns)) + list(range(nr)))
    assert batches_identical(exp, back), explain_diff(exp, back)
    assert all(exp.schema.field(i).nullable for i in range(left.num_columns))


# ------------------------------------------------------------------------------------------------ pyarrow
ARROW_TYPES = {"left": "left outer", "right": "right outer", "full": "full outer", "semi": "left semi", "anti": "left anti"}


@pytest.mark.parametrize("key_kind", ["int32", "utf8"])
@pytest.mark.parametrize("kind", list(ARROW_TYPES))
def test_reference_agrees_with_arrow_as_a_multiset(kind, key_kind):
    rng = np.random.default_rng(70 + len(key_kind))
    left, right = _side(rng, 300, [key_kind], "lrow", 0.15), _side(rng, 200, [key_kind], "rrow", 0.15)
    lidx, ridx = OJ.join_indices(left, right, [("k", "k")], kind)
    lt = pa.Table.from_batches([left.select(["k", "lrow"]).rename_columns(["lk", "lrow"])])
    rt = pa.Table.from_batches([right.select(["k", "rrow"]).rename_columns(["rk", "rrow"])])
    if kind in ("semi", "anti"):
        arrow = lt.join(rt, keys="lk", right_keys="rk", join_type=ARROW_TYPES[kind], use_threads=False)
        assert sorted(arrow.column("lrow").to_pylist()) == lidx and 0 < len(lidx) < 300
        return
    arrow = lt.join(rt, keys="lk", right_keys="rk", join_type=ARROW_TYPES[kind], coalesce_keys=False, use_threads=False)
    got = collections.Counter(zip(arrow.column("lrow").to_pylist(), arrow.column("rrow").to_pylist()))
    assert got == collections.Counter(zip(lidx, ridx))
    assert any(r is None for r in ridx) or any(l is None for l in lidx)


# ------------------------------------------------------------------------------------------------ float keys
def test_float_keys_match_by_bits_and_the_rest_is_unmatched():
    # left: +0, -0, NaN payload 1, NaN payload 2; right: -0, NaN payload 2, negative NaN payload 1, 1.5
    left = pa.RecordBatch.from_arrays([_f32([F32_POOL[0], F32_POOL[1], F32_POOL[2], F32_POOL[3]]), pa.array(np.arange(4, dtype=np.int32))],
                                      names=["k", "lrow"])
    right = pa.RecordBatch.from_arrays([_f32([F32_POOL[1], F32_POOL[3], F32_POOL[4], F32_POOL[5]]), pa.array(np.arange(4, dtype=np.int32))],
                                       names=["k", "rrow"])
    keys = [("k", "k")]
    assert _rows(*OJ.join_indices(left, right, keys, "inner")) == [(1, 0), (3, 1)]            # -0 with -0, payload 2 with payload 2
    assert _rows(*OJ.join_indices(left, right, keys, "left")) == [(0, None), (1, 0), (2, None), (3, 1)]
    assert _rows(*OJ.join_indices(left, right, keys, "right")) == [(1, 0), (3, 1), (None, 2), (None, 3)]
    assert _rows(*OJ.join_indices(left, right, keys, "full")) == [(0, None), (1, 0), (2, None), (3, 1), (None, 2), (None, 3)]
    assert OJ.join_indices(left, right, keys, "semi") == ([1, 3], None)
    assert OJ.join_indices(left, right, keys, "anti") == ([0, 2], None)                      # +0 does not match -0
    exp = OJ.join(left, right, keys, "full")[2]
    assert exp.column(0).null_count == 2 and exp.column(2).null_count == 2


# ------------------------------------------------------------------------------------------------ the operator
def _dimension(n):
    rng = np.random.default_rng(5)
    return pa.RecordBatch.from_arrays([pa.array(rng.integers(0, 60, n).astype(np.int32)), pa.array([f"name{i}" for i in range(n)])],
                                      names=["id", "name"])


def _run_join(left, right, kind, max_rows, join_fn):
    keys = join_plan(parse_select("select * from read_files('a') l join read_files('b') r on r.id = l.id"))
    ex_l = ExchangeOperator("operator_l_exchange", ["operator_join_producer"])
    ex_r = ExchangeOperator("operator_r_exchange", ["operator_join_producer"])
    ex_out = ExchangeOperator("operator_join_exchange", ["operator_p2_producer"])
    for ex, batches, alias in ((ex_l, left, "l"), (ex_r, right, "r")):
        for rid, b in enumerate(batches):
            ex.send_record(rid, b, [[alias] for _ in range(b.num_columns)])
        ex.producers_completed()
    task = JoinOperatorTask(keys, max_rows) if kind is None else JoinOperatorTask(keys, max_rows, kind)
    run = JoinTaskBuilder(join_fn).build(OperatorInstanceConfig(1, "operator_join_producer", 5, task), [ex_l, ex_r], ex_out)
    err = run()
    ex_out.producers_completed()
    got = []
    while True:
        r = ex_out.get_next_record("operator_p2_producer", 1)
        if not isinstance(r, tuple):
            break
        got.append(r)
        ex_out.operator_completed_record_processing("operator_p2_producer", r[0])
    return err, run.task, got, (ex_l, ex_r)


@pytest.mark.parametrize("kind", OJ.KINDS)
def test_join_task_runs_every_kind(kind):
    left = simple_batches(100, 4, 33)                                     # ids 0..99
    right = [_dimension(90).slice(o, 30) for o in (0, 30, 60)]            # ids among 0..59, repeated
    seen = []

    def host_join(l, la, r, ra, keys, **kw):
        seen.append(kw)
        return OJ.join(l, r, J.from_plan(keys), kw.get("kind", "inner"))[2]

    err, task, got, exchanges = _run_join(left, right, kind, 40, host_join)
    assert err is None
    assert seen == [{}] if kind == "inner" else seen == [{"kind": kind}]  # the keyword reaches join_fn, and only when it says something
    lidx, ridx, exp = OJ.join(left, right, [("id", "id")], kind)
    assert exp.num_rows > 40
    assert [r[0] for r in got] == list(range(len(got))) and len(got) == -(-exp.num_rows // 40)
    assert all(r[1].num_rows == 40 for r in got[:-1])
    left_aliases, right_aliases = [["l"], ["l"], ["l"]], [["r"], ["r"]]
    assert all(r[2] == (left_aliases if kind in ("semi", "anti") else left_aliases + right_aliases) for r in got)
    joined = R.join([r[1] for r in got])
    assert batches_identical(joined, exp), explain_diff(joined, exp)      # the rows, in the order of the kind
    if kind in ("left", "full", "anti"):
        assert None in (ridx or [None]) and exp.num_rows >= 40            # ids 60..99 have no dimension row
    assert exchanges[0].num_records() == 0 and exchanges[1].num_records() == 0
    assert task.rows_in == 190 and task.rows_out == exp.num_rows and task.records_sent == len(got)


def test_a_five_argument_join_fn_still_serves_the_default_kind():
    left, right = simple_batches(100, 4, 33), [_dimension(60)]

    def five(l, la, r, ra, keys):
        return J.join(l, r, J.from_plan(keys))[2]

    err, task, got, _ = _run_join(left, right, None, 1000, five)
    assert err is None and task.config.kind == "inner"
    exp = J.join(left, right, [("id", "id")])[2]
    assert batches_identical(R.join([r[1] for r in got]), exp)
    err, _, got, _ = _run_join(left, right, "left", 1000, five)          # ... and is told apart from one that takes the kind
    assert isinstance(err, TypeError) and got == []


def test_join_task_rejects_an_unknown_kind():
    keys = join_plan(parse_select("select * from f('a') l join f('b') r on l.id = r.id"))
    ex = [ExchangeOperator("operator_l_exchange", ["operator_join_producer"]), ExchangeOperator("operator_r_exchange", ["operator_join_producer"])]
    with pytest.raises(ValueError):
        JoinTaskBuilder(None).build(OperatorInstanceConfig(1, "operator_join_producer", 5, JoinOperatorTask(keys, 10, "sideways")), ex, None)


@pytest.mark.parametrize("kind", ["left", "full", "anti"])
def test_join_task_with_an_empty_side_sends_nothing_whatever_the_kind(kind):
    err, task, got, _ = _run_join(simple_batches(100, 4, 33), [], kind, 40, lambda *a, **k: pytest.fail("called"))
    assert err is None and got == [] and task.records_sent == 0


# ------------------------------------------------------------------------------------------------ the interface
def test_the_kind_call_is_exported():
    assert "chq_join_records_kind" in _lib.EXPORTED_SYMBOLS
    assert hasattr(_lib.lib(), "chq_join_records_kind")


def test_an_unknown_how_is_a_value_error_before_any_library_call(monkeypatch):
    monkeypatch.setattr(record_utils.L, "lib", lambda: pytest.fail("the library was called"))
    monkeypatch.setattr(record_utils, "default_context", lambda: pytest.fail("a context was created"))
    left, right = _dimension(5), _dimension(5)
    for how in ("sideways", "LEFT", "", None, 1):
        with pytest.raises(ValueError):
            record_utils.join_records(left, None, right, None, J.to_plan([("id", "id")]), how=how)
