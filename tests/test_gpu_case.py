"""GPU: CASE, COALESCE, NULLIF, BETWEEN and IN lists on the device (case.hip) against tests/case_reference.py row by row, which
the CPU tier pins to sqlite3 and pyarrow.compute.  Values, validity (no bitmap without a null), null count and -- for fixed
widths and Utf8 -- the result buffers themselves are compared: a null row's value is 0, a null string encloses no bytes."""
import decimal
import os
import re

import numpy as np
import pyarrow as pa
import pytest

import chapterhouseqe_amd as chq
from chapterhouseqe_amd import sqlparse
from chapterhouseqe_amd.sqlparse import parse_expr, parse_select
from oracle import oracle as O

from . import case_reference as R
from .cases import empty_aliases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = open(os.path.join(ROOT, "chapterhouseqe_amd", "csrc", "case.hip")).read()
_m = re.search(r"blocks > (\d+) \* (\d+) \? \1 \* \2 : blocks", _SRC)
GRID_ROWS = int(_m.group(1)) * int(_m.group(2)) * 256      # rows one pass of the row kernels' grid covers (case.hip: the cap of rows_grid, as its head comment quotes it)
SCAN_TILE = int(re.search(r"STRFN_SCAN_CHUNK\s*=\s*(\d+)", open(os.path.join(ROOT, "chapterhouseqe_amd", "csrc", "strfn_device.h")).read()).group(1))
WAVE_MODE_BYTES = int(re.search(r"CASE_WAVE_MODE_BYTES\s*=\s*(\d+)", open(os.path.join(ROOT, "chapterhouseqe_amd", "csrc", "case_device.h")).read()).group(1))
DIV_ZERO, OVERFLOW, INVALID_ARGUMENT = 21, 20, 22
D = decimal.Decimal


@pytest.fixture(scope="module")
def ctx():
    c = chq.Context(0)
    yield c
    c.close()


# ---- the batch: two columns of every family, conditions with nulls ----------------------------------------------------------
FAMILIES = {   # name -> (arrow type, row -> value of column a, row -> value of column b, a literal as SQL and as a value)
    "Int8": (pa.int8(), lambda i: i % 200 - 100, lambda i: (i * 7) % 100, None),
    "Int16": (pa.int16(), lambda i: i * 13 % 60000 - 30000, lambda i: (i * 7) % 1000, None),
    "Int32": (pa.int32(), lambda i: i * 100003 % 2**31 - 2**30, lambda i: 2**31 - 1 - i, ("7", 7)),
    "Int64": (pa.int64(), lambda i: i * 10**15 - 2**62, lambda i: 2**63 - 1 - i, ("3000000000", 3000000000)),
    "UInt8": (pa.uint8(), lambda i: i % 256, lambda i: 255 - i % 256, None),
    "UInt16": (pa.uint16(), lambda i: i * 13 % 65536, lambda i: 65535 - i % 65536, None),
    "UInt32": (pa.uint32(), lambda i: i * 100003 % 2**32, lambda i: 2**32 - 1 - i, None),
    "UInt64": (pa.uint64(), lambda i: i * 10**15, lambda i: 2**64 - 1 - i, None),
    "Float16": (pa.float16(), lambda i: np.float16(i % 512 * 0.25 - 64), lambda i: np.float16((i * 3) % 97), None),
    "Float32": (pa.float32(), lambda i: float(np.float32(i * 0.37 - 50)), lambda i: float(np.float32(1.0 / (i + 1))), ("1.5", 1.5)),
    "Float64": (pa.float64(), lambda i: i * 0.1 - 1, lambda i: 1e300 / (i + 1), None),
    "Date32": (pa.date32(), lambda i: 19000 + i, lambda i: i - 5, None),
    "Timestamp": (pa.timestamp("s"), lambda i: 2**40 + i, lambda i: -2**40 + i, None),
    "Decimal128": (pa.decimal128(30, 2), lambda i: D(2**70 + i) / 100, lambda i: D(-i) / 100, None),
    "Boolean": (pa.bool_(), lambda i: i % 2 == 0, lambda i: i % 3 == 0, ("true", True)),
    "Utf8": (pa.utf8(), lambda i: ["", "a", "héllo", "日本語", "x" * 40, "Zz"][i % 6], lambda i: f"b{i}", ("'lit'", "lit")),
}


def plain(arr):
    """to_pylist, with dates and timestamps as the integers they were built from"""
    if pa.types.is_date32(arr.type):
        arr = arr.cast(pa.int32())
    elif pa.types.is_timestamp(arr.type):
        arr = arr.cast(pa.int64())
    return arr.to_pylist()


def build(name, typ, vals):
    if pa.types.is_date32(typ):
        return pa.array(vals, pa.int32()).cast(typ)
    if pa.types.is_timestamp(typ):
        return pa.array(vals, pa.int64()).cast(typ)
    if pa.types.is_float16(typ):
        return pa.array([None if v is None else np.float16(v) for v in vals], typ)
    return pa.array(vals, typ)


def make_batch(n, families=tuple(FAMILIES), all_null=False):
    """c1, c2: Boolean with nulls; k: Int32 = row % 11; id: Int32 = row; a_<F>, b_<F>: nulls in both, b = a on every fifth row"""
    cols = {"c1": pa.array([None if i % 5 == 3 else i % 3 == 0 for i in range(n)], pa.bool_()),
            "c2": pa.array([None if i % 7 == 2 else i % 2 == 0 for i in range(n)], pa.bool_()),
            "k": pa.array([i % 11 for i in range(n)], pa.int32()), "id": pa.array(list(range(n)), pa.int32())}
    for name in families:
        typ, fa, fb, _ = FAMILIES[name]
        a = [None if all_null or i % 6 == 1 else fa(i) for i in range(n)]
        b = [None if all_null or i % 3 == 1 else (fa(i) if i % 5 == 0 else fb(i)) for i in range(n)]
        cols[f"a_{name}"], cols[f"b_{name}"] = build(name, typ, a), build(name, typ, b)
    return pa.RecordBatch.from_arrays(list(cols.values()), names=list(cols))


def lists(host):
    return {name: plain(host.column(name)) for name in host.schema.names}


# ---- comparing a result -----------------------------------------------------------------------------------------------------
def check_array(arr, want, typ, what):
    n = len(want)
    assert arr.type == typ, (what, arr.type, typ)
    assert len(arr) == n and arr.offset == 0, what
    nulls = sum(w is None for w in want)
    assert arr.null_count == nulls, (what, arr.null_count, nulls)
    if nulls:
        assert arr.is_valid().to_pylist() == [w is not None for w in want], what
    else:
        assert arr.buffers()[0] is None, what
    got = plain(arr)
    bad = [i for i in range(n) if got[i] != want[i]][:8]
    assert not bad, f"{what}: first differences at {bad}: {[(got[i], want[i]) for i in bad]}"
    if n == 0:
        return
    if typ == pa.utf8():      # the buffers: offsets from 0, a null row encloses nothing, no byte beyond the total
        enc = [b"" if w is None else w.encode() for w in want]
        offs = np.frombuffer(arr.buffers()[1], np.int32, n + 1)
        exp = np.zeros(n + 1, np.int64)
        np.cumsum([len(e) for e in enc], out=exp[1:])
        assert np.array_equal(offs, exp), (what, "offsets")
        total = int(exp[-1])
        assert (arr.buffers()[2].to_pybytes()[:total] if total else b"") == b"".join(enc), (what, "bytes")
    elif typ != pa.bool_() and nulls:      # a null row's value is 0
        raw = np.frombuffer(arr.buffers()[1], np.uint8, n * typ.byte_width).reshape(n, typ.byte_width)
        assert not raw[[w is None for w in want]].any(), (what, "the values of null rows")


def check_value(c, rec, host, sql, want, typ, what):
    arr, is_scalar = chq.compute_value(rec, empty_aliases(host), parse_expr(sql), ctx=c)
    assert not is_scalar, (what, sql)
    check_array(arr, want, typ, f"{what}: {sql}")


def on_both(c, host, forms, what, offsets=()):
    """every form on the device batch and on the host batch, then on sliced views of both at `offsets`"""
    dev = chq.DeviceRecordBatch.from_host(host, c)
    cols = lists(host)
    n = host.num_rows
    wants = [(sql, typ, f(cols, n)) for sql, typ, f in forms]
    for sql, typ, want in wants:
        check_value(c, dev, host, sql, want, typ, what)
        check_value(c, host, host, sql, want, typ, what + ", host record")
    for off in offsets:
        ln = n - off - (off % 3)
        for sql, typ, want in wants:
            check_value(c, dev.slice(off, ln), host.slice(off, ln), sql, want[off:off + ln], typ, f"{what}, device view ({off}, {ln})")
            check_value(c, host.slice(off, ln), host.slice(off, ln), sql, want[off:off + ln], typ, f"{what}, host slice ({off}, {ln})")


def family_forms(name):
    typ, _, _, lit = FAMILIES[name]
    a, b = f"a_{name}", f"b_{name}"
    forms = [
        (f"case when c1 then {a} else {b} end", typ, lambda c, n: R.case_when([c["c1"]], [c[a]], c[b])),
        (f"case when c1 then {a} when c2 then {b} end", typ, lambda c, n: R.case_when([c["c1"], c["c2"]], [c[a], c[b]])),
        (f"coalesce({a}, {b})", typ, lambda c, n: R.coalesce(c[a], c[b])),
        (f"nullif({a}, {b})", typ, lambda c, n: R.nullif(c[a], c[b])),
        (f"case k when 1 then {a} when 4 then {b} when 1 then {b} else {a} end", typ,
         lambda c, n: R.simple_case(c["k"], [[1] * n, [4] * n, [1] * n], [c[a], c[b], c[b]], c[a])),
    ]
    if lit is not None:
        sql, val = lit
        forms.append((f"case when c2 then {sql} when c1 then {a} end", typ, lambda c, n: R.case_when([c["c2"], c["c1"]], [[val] * n, c[a]])))
        forms.append((f"coalesce({a}, {sql})", typ, lambda c, n: R.coalesce(c[a], [val] * n)))
        forms.append((f"nullif({a}, {sql})", typ, lambda c, n: R.nullif(c[a], [val] * n)))
    return forms


def when_chain(count, col="a_Int32", alt="b_Int32", els=True):
    """`count` WHENs on k (0 .. 10): odd ones give `col`, even ones `alt`"""
    sql = "case " + " ".join(f"when k = {j} then {col if j % 2 else alt}" for j in range(count)) + (f" else {col}" if els else "") + " end"
    f = lambda c, n: R.case_when([[v == j for v in c["k"]] for j in range(count)], [c[col] if j % 2 else c[alt] for j in range(count)], c[col] if els else None)
    return sql, f


# ---- every family ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(FAMILIES))
def test_every_family_on_device_host_and_views(ctx, name):
    host = make_batch(200, (name,))
    on_both(ctx, host, family_forms(name), name, offsets=(1, 7, 65))


@pytest.mark.parametrize("name", ["Int32", "Utf8", "Boolean", "Decimal128"])
def test_all_null_branches(ctx, name):
    host = make_batch(130, (name,), all_null=True)
    on_both(ctx, host, family_forms(name)[:4], f"{name}, all null", offsets=(7,))


@pytest.mark.parametrize("rows", [0, 1, 63, 64, 65, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1])
def test_row_counts(ctx, rows):
    host = make_batch(rows, ("Int32", "Utf8", "Boolean", "Int8", "Decimal128"))
    forms = [family_forms(f)[k] for f, k in (("Int32", 0), ("Int32", 1), ("Utf8", 0), ("Utf8", 5), ("Boolean", 1), ("Int8", 2), ("Decimal128", 3))]
    on_both(ctx, host, forms, f"{rows} rows")


def test_one_grid_pass_and_65_rows(ctx):
    """the row kernels walk their rows in passes of GRID_ROWS: the rows of the second pass, Int32 and Utf8 (expectations by numpy)"""
    n = GRID_ROWS + 65
    ids = np.arange(n, dtype=np.int32)
    c1 = ids % 3 == 0
    a = (ids * 7 % 1000).astype(np.int32)
    valid_a = ids % 6 != 3
    s = np.char.add("r", (ids % 977).astype(str))
    host = pa.RecordBatch.from_arrays([pa.array(c1), pa.array(a, mask=~valid_a), pa.array(ids), pa.array(s, pa.utf8())], names=["c1", "a", "id", "s"])
    dev = chq.DeviceRecordBatch.from_host(host, ctx)
    arr, _ = chq.compute_value(dev, empty_aliases(host), parse_expr("case when c1 then a else id end"), ctx=ctx)
    assert arr.type == pa.int32() and arr.null_count == int((c1 & ~valid_a).sum())
    got = np.frombuffer(arr.buffers()[1], np.int32, n)
    assert np.array_equal(got, np.where(c1, np.where(valid_a, a, 0), ids))
    assert np.array_equal(np.unpackbits(np.frombuffer(arr.buffers()[0], np.uint8), bitorder="little")[:n].astype(bool), ~(c1 & ~valid_a))
    arr, _ = chq.compute_value(dev, empty_aliases(host), parse_expr("case when c1 then s else 'no' end"), ctx=ctx)
    want = np.where(c1, s, "no")
    assert arr.null_count == 0 and arr.buffers()[0] is None
    lens = np.char.str_len(want)
    exp = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=exp[1:])
    assert np.array_equal(np.frombuffer(arr.buffers()[1], np.int32, n + 1), exp)
    assert arr.buffers()[2].to_pybytes()[:int(exp[-1])] == "".join(want.tolist()).encode()


# ---- branches that are literals and computed, casts, WHEN counts -----------------------------------------------------------------
def test_literal_computed_and_cast_branches(ctx):
    host = make_batch(300, ("Int8", "Int32", "Float32", "Float64", "Utf8", "Boolean"))
    f32 = lambda v: None if v is None else float(np.float32(v))
    forms = [
        ("case when c1 then 1 else 2 end", pa.int32(), lambda c, n: R.case_when([c["c1"]], [[1] * n], [2] * n)),
        ("case when c1 then 'yes' when c2 then '' end", pa.utf8(), lambda c, n: R.case_when([c["c1"], c["c2"]], [["yes"] * n, [""] * n])),
        ("case when c1 then k + 1 else k * 2 end", pa.int32(), lambda c, n: R.case_when([c["c1"]], [[v + 1 for v in c["k"]]], [v * 2 for v in c["k"]])),
        ("case when k > 5 then a_Float32 * 2.0 else 0.5 end", pa.float32(),
         lambda c, n: R.case_when([[v > 5 for v in c["k"]]], [[f32(None if v is None else np.float32(v) * np.float32(2)) for v in c["a_Float32"]]], [0.5] * n)),
        # Int8, Int32 and Float32 meet in Float32: every branch is cast
        ("case when c1 then a_Int8 when c2 then a_Int32 else a_Float32 end", pa.float32(),
         lambda c, n: R.case_when([c["c1"], c["c2"]], [[f32(v) for v in c["a_Int8"]], [f32(v) for v in c["a_Int32"]]], c["a_Float32"])),
        ("coalesce(a_Int8, a_Int32, 7)", pa.int32(), lambda c, n: R.coalesce(c["a_Int8"], c["a_Int32"], [7] * n)),
        ("coalesce(a_Float32, a_Float64)", pa.float64(), lambda c, n: R.coalesce(c["a_Float32"], c["a_Float64"])),
        ("nullif(a_Int8, a_Int32)", pa.int8(), lambda c, n: R.nullif(c["a_Int8"], c["a_Int32"])),
        # conditions that are computed, literal, LIKE and IS NULL; a CASE inside a CASE, under a string function, in a comparison
        # (upper() is ASCII-only: 'héllo' -> 'HéLLO')
        ("case when a_Utf8 like '%l%' then upper(a_Utf8) when a_Utf8 is null then 'none' else a_Utf8 || '!' end", pa.utf8(),
         lambda c, n: [("none" if v is None else "".join(ch.upper() if ch.isascii() else ch for ch in v) if "l" in v else v + "!") for v in c["a_Utf8"]]),
        ("case when false then 1 when true then k end", pa.int32(), lambda c, n: list(c["k"])),
        ("case when c1 then case when c2 then 1 else 2 end else 3 end", pa.int32(),
         lambda c, n: R.case_when([c["c1"]], [R.case_when([c["c2"]], [[1] * n], [2] * n)], [3] * n)),
        ("case when c1 then a_Int32 end + 1 > k", pa.bool_(), lambda c, n: [None if not x or v is None else v + 1 > kk for x, v, kk in zip(c["c1"], c["a_Int32"], c["k"])]),
        ("case when c1 then a_Utf8 else 'a' end = 'a'", pa.bool_(),
         lambda c, n: [None if w is None else w == "a" for w in R.case_when([c["c1"]], [c["a_Utf8"]], ["a"] * n)]),
        ("case when a_Boolean then c1 when c2 then false else b_Boolean end", pa.bool_(),
         lambda c, n: R.case_when([c["a_Boolean"], c["c2"]], [c["c1"], [False] * n], c["b_Boolean"])),
    ]
    on_both(ctx, host, forms, "branches", offsets=(1, 65))


@pytest.mark.parametrize("count", [1, 2, 8, 9, 11])
def test_when_counts(ctx, count):
    host = make_batch(200, ("Int32", "Utf8"))
    forms = []
    for els in (True, False):
        sql, f = when_chain(count, els=els)
        forms.append((sql, pa.int32(), f))
    sql, f = when_chain(count, "a_Utf8", "b_Utf8", els=False)
    forms.append((sql, pa.utf8(), f))
    # conditions that can fail on data are guarded, so the masks are built WHEN by WHEN: `id % 11` is checked arithmetic
    sql = "case " + " ".join(f"when id % 11 = {j} then {'a_Int32' if j % 2 else 'b_Int32'}" for j in range(count)) + " end"
    forms.append((sql, pa.int32(), when_chain(count, els=False)[1]))
    on_both(ctx, host, forms, f"{count} WHENs", offsets=(7,))


def test_utf8_wave_mode_of_the_gather(ctx):
    """64 rows whose chosen strings hold the threshold exactly (lane per row), one byte more (wave per row), with empty and null rows"""
    per = WAVE_MODE_BYTES // 64
    for extra in (0, 1, 3000):
        s = ["ab"[i % 2] * per for i in range(64)]
        s[17] += "q" * extra
        t = [None if i % 9 == 4 else "" if i % 9 == 5 else "T" * (i % 70) for i in range(64)]
        pick = [True] * 64
        rows = s + t + s[:30]
        other = t + s + t[:30]
        cond = pick + [i % 2 == 0 for i in range(64)] + [True] * 30
        host = pa.RecordBatch.from_arrays([pa.array(rows, pa.utf8()), pa.array(other, pa.utf8()), pa.array(cond)], names=["s", "t", "c"])
        want = R.case_when([cond], [rows], other)
        dev = chq.DeviceRecordBatch.from_host(host, ctx)
        check_value(ctx, dev, host, "case when c then s else t end", want, pa.utf8(), f"wave mode, {extra} over")
        check_value(ctx, dev.slice(1, 150), host.slice(1, 150), "case when c then s else t end", want[1:151], pa.utf8(), f"wave mode, {extra} over, view")


# ---- lazy errors --------------------------------------------------------------------------------------------------------------------
def lazy_batch(n=300):
    a = [i * 3 - 100 for i in range(n)]
    b = [None if i % 13 == 5 else i % 4 for i in range(n)]                     # zeros on every fourth row
    big = [2**31 - 1 if i >= 100 else i for i in range(n)]
    z = [0 if i % 10 == 3 else i % 7 + 1 for i in range(n)]
    bn = [None if i == 43 else v for i, v in enumerate(z)]                      # = z, but null on one of z's zero rows
    return pa.RecordBatch.from_arrays([pa.array(a, pa.int32()), pa.array(b, pa.int32()), pa.array(big, pa.int32()), pa.array(z, pa.int32()), pa.array(bn, pa.int32()),
                                       pa.array(list(range(n)), pa.int32()), pa.array([i % 3 == 0 for i in range(n)])], names=["a", "b", "big", "z", "bn", "id", "c"])


def status_of(c, rec, host, sql):
    with pytest.raises(chq.ChqError) as ei:
        chq.compute_value(rec, empty_aliases(host), parse_expr(sql), ctx=c)
    return ei.value.code


def test_lazy_errors_guarded_branches_succeed(ctx):
    host = lazy_batch()
    n = host.num_rows
    col = lists(host)
    a, b, big, z, ids = col["a"], col["b"], col["big"], col["z"], col["id"]
    nz = lambda i: None if b[i] is None else b[i] != 0
    forms = [
        ("case when b <> 0 then a / b else 0 end", pa.int32(), lambda c, m: R.lazy_case(n, [nz], [lambda i: R.checked("/", a[i], b[i])], lambda i: 0)),
        ("case when b <> 0 then a % b end", pa.int32(), lambda c, m: R.lazy_case(n, [nz], [lambda i: R.checked("%", a[i], b[i])])),
        ("case when id < 100 then big * 2 else big end", pa.int32(), lambda c, m: R.lazy_case(n, [lambda i: ids[i] < 100], [lambda i: R.checked("*", big[i], 2)], lambda i: big[i])),
        ("case when id >= 100 then 0 else big + big end", pa.int32(), lambda c, m: R.lazy_case(n, [lambda i: ids[i] >= 100], [lambda i: 0], lambda i: R.checked("+", big[i], big[i]))),
        # a guarded CONDITION: the division runs only where the first WHEN was not true
        ("case when z = 0 then 0 when a / z > 2 then 1 else 2 end", pa.int32(),
         lambda c, m: R.lazy_case(n, [lambda i: z[i] == 0, lambda i: R.checked("/", a[i], z[i]) > 2], [lambda i: 0, lambda i: 1], lambda i: 2)),
        ("coalesce(case when b <> 0 then a / b end, a)", pa.int32(), lambda c, m: R.coalesce(R.lazy_case(n, [nz], [lambda i: R.checked("/", a[i], b[i])]), a)),
    ]
    on_both(ctx, host, forms, "guarded", offsets=(1, 65))
    # inside a filter: the guard holds there too
    dev = chq.DeviceRecordBatch.from_host(host, ctx)
    got = chq.filter_record(dev, empty_aliases(host), parse_expr("case when b <> 0 then a / b > 10 else false end"), ctx=ctx).to_host()
    keep = R.lazy_case(n, [nz], [lambda i: R.checked("/", a[i], b[i]) > 10], lambda i: False)
    assert got.equals(host.filter(pa.array([k is True for k in keep], pa.bool_())))


def test_lazy_errors_count_on_taken_rows(ctx):
    host = lazy_batch()
    dev = chq.DeviceRecordBatch.from_host(host, ctx)
    n = host.num_rows
    col = lists(host)
    for rec in (dev, host, dev.slice(7, 200)):
        assert status_of(ctx, rec, host, "case when c then a / b end") == DIV_ZERO                   # a taken row divides by zero
        assert status_of(ctx, rec, host, "case when b = 0 then a / b else 0 end") == DIV_ZERO
        assert status_of(ctx, rec, host, "case when c then 0 else a / b end") == DIV_ZERO            # in the ELSE
        assert status_of(ctx, rec, host, "case when id > 150 then big * 2 else big end") == OVERFLOW
        assert status_of(ctx, rec, host, "case when id < 101 then big * 2 else big end") == OVERFLOW      # one taken row is enough
        # the first condition is evaluated on every row
        assert status_of(ctx, rec, host, "case when a / b > 0 then 1 end") == DIV_ZERO
        # a NULL earlier condition does not guard: bn is null on row 43, where z is 0
        assert status_of(ctx, rec, host, "case when bn = 0 then 0 when a / z > 2 then 1 else 2 end") == DIV_ZERO
        # conditions are evaluated before results: the overflow of r1 is not what is reported
        assert status_of(ctx, rec, host, "case when c then big * 2 when a / b > 0 then 1 end") == DIV_ZERO
    # the reference agrees on which raise
    with pytest.raises(R.DivideByZero):
        R.lazy_case(n, [lambda i: None if col["bn"][i] is None else col["bn"][i] == 0, lambda i: R.checked("/", col["a"][i], col["z"][i]) > 2], [lambda i: 0, lambda i: 1])
    with pytest.raises(R.Overflow):
        R.lazy_case(n, [lambda i: col["id"][i] > 150], [lambda i: R.checked("*", col["big"][i], 2)])


# ---- the forms inside the record calls --------------------------------------------------------------------------------------------------
PREDICATES = ["case when c1 then a_Int32 > 0 else c2 end", "coalesce(c1, c2)", "case when k < 5 then a_Utf8 else b_Utf8 end like 'b%'",
              "nullif(k, 3) is null", "k in (1, 4, 9)", "a_Int32 not between 0 and 1000000000", "a_Utf8 in ('a', 'Zz', '')"]


def predicate_mask(cols, n, sql):
    c = cols
    if sql == PREDICATES[0]:
        return R.case_when([c["c1"]], [[None if v is None else v > 0 for v in c["a_Int32"]]], c["c2"])
    if sql == PREDICATES[1]:
        return R.coalesce(c["c1"], c["c2"])
    if sql == PREDICATES[2]:
        return [None if w is None else w.startswith("b") for w in R.case_when([[v < 5 for v in c["k"]]], [c["a_Utf8"]], c["b_Utf8"])]
    if sql == PREDICATES[3]:
        return [v == 3 for v in c["k"]]
    if sql == PREDICATES[4]:
        return R.in_list(c["k"], [1, 4, 9])
    if sql == PREDICATES[5]:
        return R.between(c["a_Int32"], [0] * n, [1000000000] * n, True)
    return R.in_list(c["a_Utf8"], ["a", "Zz", ""])


def kept(host, mask):
    return host.filter(pa.array([m is True for m in mask], pa.bool_()))


@pytest.mark.parametrize("sql", PREDICATES)
def test_filter_record_and_filter_records(ctx, sql):
    hosts = [make_batch(n, ("Int32", "Utf8")) for n in (150, 64, 0, 301)]
    al = empty_aliases(hosts[0])
    wants = [kept(h, predicate_mask(lists(h), h.num_rows, sql)) for h in hosts]
    for h, want in zip(hosts, wants):
        assert chq.filter_record(chq.DeviceRecordBatch.from_host(h, ctx), al, parse_expr(sql), ctx=ctx).to_host().equals(want), (sql, h.num_rows)
        assert chq.filter_record(h, al, parse_expr(sql), ctx=ctx).equals(want), (sql, h.num_rows, "host")
    got = chq.filter_records([chq.DeviceRecordBatch.from_host(h, ctx) for h in hosts], al, parse_expr(sql), ctx=ctx)
    assert [g.to_host().equals(w) for g, w in zip(got, wants)] == [True] * len(hosts), sql
    got = chq.filter_records(hosts, al, parse_expr(sql), ctx=ctx, device_result=False)
    assert [g.equals(w) for g, w in zip(got, wants)] == [True] * len(hosts), sql
    view = chq.DeviceRecordBatch.from_host(hosts[3], ctx).slice(7, 200)
    assert chq.filter_record(view, al, parse_expr(sql), ctx=ctx).to_host().equals(kept(hosts[3].slice(7, 200), predicate_mask(lists(hosts[3].slice(7, 200)), 200, sql)))


def test_project_record_and_filter_project_record(ctx):
    host = make_batch(257, ("Int32", "Utf8", "Float32"))
    cols = lists(host)
    n = host.num_rows
    sel = parse_select("select case when c1 then a_Int32 else k end as v, case k when 0 then 'zero' when 1 then a_Utf8 end as s, coalesce(a_Float32, 0.5), id, "
                       "nullif(k, 3) as nk, k between 2 and 4 as bt, case when c2 then c1 end as cb from x")
    wants = [R.case_when([cols["c1"]], [cols["a_Int32"]], cols["k"]), R.simple_case(cols["k"], [[0] * n, [1] * n], [["zero"] * n, cols["a_Utf8"]]),
             R.coalesce(cols["a_Float32"], [0.5] * n), cols["id"], R.nullif(cols["k"], [3] * n), R.between(cols["k"], [2] * n, [4] * n), R.case_when([cols["c2"]], [cols["c1"]])]
    types = [pa.int32(), pa.utf8(), pa.float32(), pa.int32(), pa.int32(), pa.bool_(), pa.bool_()]
    for rec in (chq.DeviceRecordBatch.from_host(host, ctx), host):
        out = chq.project_record(sel.projection, rec, empty_aliases(host), ctx=ctx, device_result=False)
        assert out.schema.names == ["v", "s", "unnamed_0", "id", "nk", "bt", "cb"]
        for k, (want, typ) in enumerate(zip(wants, types)):
            check_array(out.column(k), want, typ, f"select item {k}")
            assert out.schema.field(k).nullable == any(w is None for w in want), k      # nullable iff it holds a null
    mask = predicate_mask(cols, n, PREDICATES[0])
    rows = [i for i in range(n) if mask[i] is True]
    out = chq.filter_project_record(parse_expr(PREDICATES[0]), sel.projection, chq.DeviceRecordBatch.from_host(host, ctx), empty_aliases(host), ctx=ctx).to_host()
    assert out.num_rows == len(rows)
    for k, (want, typ) in enumerate(zip(wants, types)):
        check_array(out.column(k), [want[i] for i in rows], typ, f"filter + select item {k}")
    # a plain predicate in front of CASE items, and a CASE predicate in front of plain items
    out = chq.filter_project_record(parse_expr("k > 5"), sel.projection[:2], host, empty_aliases(host), ctx=ctx)
    rows = [i for i in range(n) if cols["k"][i] > 5]
    check_array(out.column(0), [wants[0][i] for i in rows], pa.int32(), "plain predicate, CASE item")
    out = chq.filter_project_record(parse_expr(PREDICATES[4]), parse_select("select id, k + 1 from x").projection, host, empty_aliases(host), ctx=ctx)
    assert plain(out.column(0)) == [i for i in range(n) if cols["k"][i] in (1, 4, 9)]


# ---- BETWEEN and IN against their spelled-out forms through the CPU implementation of the reference -----------------------------------
SUGAR = [("a_Int32", "b_Int32", "k"), ("k", "2", "a_Int8"), ("a_Float32", "0.5", "b_Float32"), ("a_Utf8", "'a'", "b_Utf8"), ("k + 1", "3", "k * 2"), ("a_Int8", "a_Int32", "100")]
LISTS = [("k", ["1"]), ("k", ["1", "4", "9", "10"]), ("a_Int8", ["100", "7", "3000000000"]), ("a_Float32", ["1.5", "2"]), ("a_Utf8", ["'a'", "'héllo'", "''"]),
         ("k * 2", ["(4)", "8"]), ("c1", ["true"]), ("k", [str(j) for j in range(32)])]


def test_between_and_in_equal_their_spelled_out_forms(ctx):
    host = make_batch(200, ("Int8", "Int32", "Float32", "Utf8"))
    dev = chq.DeviceRecordBatch.from_host(host, ctx)
    al = empty_aliases(host)
    pairs = [(f"{x} {'not ' if neg else ''}between {lo} and {hi}", R.between_sql(x, lo, hi, neg)) for x, lo, hi in SUGAR for neg in (False, True)]
    pairs += [(f"{x} {'not ' if neg else ''}in ({', '.join(items)})", R.in_list_sql(x, items, neg)) for x, items in LISTS for neg in (False, True)]
    for sugar, spelled in pairs:
        want = O.compute_value(host, al, parse_expr(spelled))[0]
        for rec in (dev, host, dev.slice(7, 130)):
            got = chq.compute_value(rec, al, parse_expr(sugar), ctx=ctx)[0]
            exp = want.slice(7, 130) if rec is not dev and rec is not host else want
            assert got.equals(exp) and got.null_count == exp.null_count, (sugar, got.to_pylist()[:20], exp.to_pylist()[:20])
            same = chq.compute_value(rec, al, parse_expr(spelled), ctx=ctx)[0]
            assert got.buffers()[1].to_pybytes()[: (len(got) + 7) // 8] == same.buffers()[1].to_pybytes()[: (len(got) + 7) // 8], sugar      # bit for bit
        assert O.filter_record(host, al, parse_expr(spelled)).equals(chq.filter_record(dev, al, parse_expr(sugar), ctx=ctx).to_host()), sugar
    # the same statuses: a division by zero inside x, lo or an item-free chain
    zero = pa.RecordBatch.from_arrays([pa.array([1, 2, 0], pa.int32()), pa.array([3, 4, 5], pa.int32())], names=["z", "v"])
    for sugar, spelled in (("v / z between 1 and 2", R.between_sql("v / z", "1", "2")), ("v / z in (1, 2)", R.in_list_sql("v / z", ["1", "2"])), ("v between 1 / z and 9", "")):
        assert status_of(ctx, zero, zero, sugar) == DIV_ZERO
        if spelled:
            assert status_of(ctx, zero, zero, spelled) == DIV_ZERO


# ---- project a CASE bucket, then aggregate by it ---------------------------------------------------------------------------------------------
def test_case_bucket_then_aggregate(ctx):
    host = make_batch(1000, ("Int32",))
    cols = lists(host)
    n = host.num_rows
    sel = parse_select("select case when k < 3 then 'low' when k < 8 then 'mid' when c1 then 'high' end as bucket, k * 10 as v from x")
    proj = chq.project_record(sel.projection, chq.DeviceRecordBatch.from_host(host, ctx), empty_aliases(host), ctx=ctx)
    keys, items = sqlparse.aggregate_plan(parse_select("select bucket, sum(v) as total, count(*) as rows from x group by bucket"))
    out = chq.aggregate_record(proj, [[], []], keys, items, ctx=ctx).to_host()
    bucket = R.case_when([[v < 3 for v in cols["k"]], [v < 8 for v in cols["k"]], cols["c1"]], [["low"] * n, ["mid"] * n, ["high"] * n])
    sums, counts = {}, {}
    for b, k in zip(bucket, cols["k"]):
        sums[b] = sums.get(b, 0) + k * 10
        counts[b] = counts.get(b, 0) + 1
    order = sorted(b for b in sums if b is not None) + [None]      # key order, nulls last
    assert None in sums and out.column(0).to_pylist() == order
    assert out.column(1).to_pylist() == [sums[b] for b in order] and out.column(2).to_pylist() == [counts[b] for b in order]


# ---- a Utf8 result past int32 offsets: refused before a byte is copied ---------------------------------------------------------------------
def test_utf8_byte_total_refusal(ctx):
    """forged offsets, no large allocation: two columns of two rows that claim 2^30 bytes in the row the CASE takes from each.
    The row kernel reads offsets only, the total (2^31) is checked on the host, and the gather -- which would read the bytes --
    never runs."""
    big = 2**30
    offs = pa.RecordBatch.from_arrays([pa.array([0, big, big], pa.int32()), pa.array([0, 0, big], pa.int32()), pa.array([1, 0, 0], pa.int32())], names=["so", "to", "c"])
    cond = pa.RecordBatch.from_arrays([pa.array([True, False])], names=["c"])
    up, upc = chq.DeviceRecordBatch.from_host(offs, ctx), chq.DeviceRecordBatch.from_host(cond, ctx)
    data = up.column_buffer_address(2)      # 12 bytes that are never read
    dev = chq.DeviceRecordBatch.from_device_buffers([{"name": "s", "format": "u", "values": up.column_buffer_address(0), "data": data},
                                                     {"name": "t", "format": "u", "values": up.column_buffer_address(1), "data": data},
                                                     {"name": "c", "format": "b", "values": upc.column_buffer_address(0)}], 2, ctx, keepalive=[up, upc])
    with pytest.raises(chq.ChqError) as ei:
        chq.compute_value(dev, [[], [], []], parse_expr("case when c then s else t end"), ctx=ctx)
    assert ei.value.code == INVALID_ARGUMENT and "int32 offsets" in str(ei.value) and str(2**31) in str(ei.value)
