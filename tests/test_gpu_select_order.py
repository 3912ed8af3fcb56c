"""GPU: the order in which the select items of one list are read, named and fail, against the CPU oracle.  The reference
evaluates the items one after the other (record_projection.rs:16-76), so an earlier item's data-dependent error (division
by zero, overflow) beats a later item's static one (unknown column, QualifiedWildcard), and inside one item the completed
sub-trees' data errors beat its own static error.  Every list goes through project_record and filter_project_record, on a
device and on a host batch (the host projection path and the single-pass kernel must decline or agree); the error CODE is
compared, or on success the whole batch with column names and nullability.

3-row Int32 batches, the smallest that tell the orderings apart: `z` has one failing row that is neither first nor last,
`m` one overflowing row."""
import numpy as np
import pyarrow as pa
import pytest

import chapterhouseqe_amd as chq
from chapterhouseqe_amd.sqlparse import parse_select
from oracle import oracle as O

from .cases import empty_aliases
from .helpers import batches_identical, explain_diff

pytestmark = pytest.mark.gpu

REC = pa.RecordBatch.from_arrays(
    [pa.array(np.array(v, dtype=np.int32)) for v in ([1, 2, 3], [1, 0, 1], [2147483647, 1, 1])], names=["a", "z", "m"])

# (select list, the oracle's status on the 3-row batch: None = success)
LISTS = [
    ("a / z as q, nosuch", 21),                       # divide by zero before column not found
    ("nosuch, a / z as q", 7),
    ("a, (a / z) + nosuch as r", 21),                 # the item's own completed sub-tree before its static error
    ("m + m as s, (a / z) + nosuch as r", 20),        # ... and an earlier item's overflow before both
    ("a + 1 as ok, (a / z) + nosuch as r", 21),
    ("a + 1 as ok, a + nosuch as r", 7),
    ("a / z as q, t.*", 21),
    ("a + 1 as ok, t.*", 11),                         # not implemented: SelectItem::QualifiedWildcard
    ("a / z as q, m + m as s", 21),
    ("a, (m + m) + (a / z) as r", 20),
    ("a + 1, a, 7, a * 2 as d, *", 22),               # a literal is a length-1 column: length mismatch on 3 rows
    ("a + 1, a, a * 2 as d, *", None),
]
PENDING = [s for s, _ in LISTS if "(a / z) + nosuch" in s]   # a static error held back behind data-dependent ones


@pytest.fixture(scope="module")
def ctxs():
    cs = []
    for fuse in (1, 2):
        c = chq.Context(0)
        c.set_option("fuse", fuse)
        cs.append(c)
    yield cs
    for c in cs:
        c.close()


def outcome(call):
    try:
        return None, call()
    except (chq.ChqError, O.OracleError) as e:
        return e.code, None


def agree(what, got, exp):
    (gcode, gbatch), (xcode, xbatch) = got, exp
    assert gcode == xcode, f"{what}: status {gcode}, the oracle's {xcode}"
    if xbatch is not None:
        assert batches_identical(gbatch, xbatch, nan_payload=True), f"{what}:\n{explain_diff(gbatch, xbatch)}"


def check_all_entries(ctxs, rec, select_list):
    """project_record and filter_project_record (fuse = 1 and 2), device and host batch; returns the oracle's outcome of
    project_record.  After a failing call the same context serves a successful one."""
    al = empty_aliases(rec)
    proj = parse_select(f"select {select_list} from t")
    both = parse_select(f"select {select_list} from t where a > 0")
    fine = parse_select("select a, a + 1 as n from t where a > 0")
    exp_p = outcome(lambda: O.project_record(proj.projection, rec, al))
    exp_fp = outcome(lambda: O.project_record(both.projection, O.filter_record(rec, al, both.selection), al))
    exp_fine = outcome(lambda: O.project_record(fine.projection, O.filter_record(rec, al, fine.selection), al))
    assert exp_fine[0] is None
    for device in (True, False):
        def run(c, f):
            src = chq.DeviceRecordBatch.from_host(rec, c) if device else rec
            got = f(src, c)
            return got.to_host() if device else got
        where = "device" if device else "host"
        entries = [(f"project_record, {where} batch", ctxs[0], proj, exp_p,
                    lambda src, c: chq.project_record(proj.projection, src, al, ctx=c))]
        for c, fuse in zip(ctxs, (1, 2)):
            entries.append((f"filter_project_record fuse={fuse}, {where} batch", c, both, exp_fp,
                            lambda src, c: chq.filter_project_record(both.selection, both.projection, src, al, ctx=c)))
        for what, c, _sel, exp, f in entries:
            got = outcome(lambda: run(c, f))
            agree(f"{what}: select {select_list} ({rec.num_rows} rows)", got, exp)
            if got[0] is not None:   # the context stays usable
                again = outcome(lambda: run(c, lambda src, c: chq.filter_project_record(fine.selection, fine.projection, src, al, ctx=c)))
                agree(f"{what}: the call after the failing one", again, exp_fine)
    return exp_p


@pytest.mark.parametrize("select_list,code", LISTS, ids=[s for s, _ in LISTS])
def test_item_order_decides_which_error_wins(ctxs, select_list, code):
    exp_code, exp = check_all_entries(ctxs, REC, select_list)
    assert exp_code == code   # (the oracle's answer, as recorded when these lists were chosen)
    if code is None:
        assert exp.schema.names == ["unnamed_0", "a", "d", "a", "z", "m"]   # unnamed_N counts the identifier item too


def test_literal_item_on_one_row(ctxs):
    """on a 1-row batch the literal's length-1 column has the batch's length"""
    check_all_entries(ctxs, REC.slice(0, 1), "a + 1, a, 7, a * 2 as d, *")


@pytest.mark.parametrize("select_list", PENDING)
def test_no_rows_no_validation(ctxs, select_list):
    """0 rows: nothing is evaluated, so nothing can fail on data and the static error is what is left"""
    exp_code, _ = check_all_entries(ctxs, REC.slice(0, 0), select_list)
    assert exp_code == 7
