"""CPU tier of the Parquet writer: its layout unit (csrc/parquet_layout.cpp: page size, page cuts, level runs, Thrift page
headers, chunk offsets, statistics bytes, the footer) without a GPU.  tests/parquet_layout_main.cpp makes what the kernels
would hand over with plain loops, builds whole files with the layout and footer functions under the host sanitizers and
writes them into a directory; here every file is read by pyarrow (values, nulls, nullability, null_count / min / max per
chunk), page by page by tests/parquet_unpage.py, and by the library's own metadata reader, and compared with the table the
program was told to write -- the same rules of the row number on both sides.  tests/test_gpu_parquet_write_edges.py pins
the device encode in front of this unit."""
import io
import os
import re
import shutil
import subprocess

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

import chapterhouseqe_amd as chq
from tests import parquet_unpage as U
from tests.helpers import arrays_identical, batches_identical, explain_diff
from tests.test_parquet import parse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAGE_ROWS = 4096
CUT_ROWS = (0, 1, 4095, 4096, 4097, 3 * 4096 + 5)
ROW_GROUP_ROWS = (4097, 0, 1, 8192)          # = tests/parquet_write_cases.py ROW_GROUP_ROWS
FILES = ["cuts_%d" % n for n in CUT_ROWS] + ["widened", "page_rows_1", "page_rows_5000", "row_groups", "schema_15", "schema_16", "long_name",
                                             "long_bound", "statistics"]


@pytest.fixture(scope="module")
def written(tmp_path_factory):
    """name -> bytes of every file the program wrote, after its own checks passed under the sanitizers"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler on PATH")
    out = tmp_path_factory.mktemp("parquet_layout")
    exe = str(out / "parquet_layout_main")
    flags = ["-std=c++17", "-O0", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    src = os.path.join(ROOT, "tests", "parquet_layout_main.cpp")
    build = subprocess.run([cxx, *flags, "-static-libasan", "-static-libubsan", src, "-o", exe], capture_output=True, text=True)
    if build.returncode != 0:
        build = subprocess.run([cxx, *flags, src, "-o", exe], capture_output=True, text=True)
    if build.returncode != 0 and re.search(r"asan|ubsan|sanitize", build.stderr, re.I):
        pytest.skip("the compiler has no sanitizer runtime: " + build.stderr.strip().splitlines()[-1])
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe, str(out)], capture_output=True, text=True)
    if run.returncode != 0 and "runtime does not come first" in run.stderr:
        pytest.skip("this environment preloads a library in front of the sanitizer runtime: " + run.stderr.strip().splitlines()[0])
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    m = re.fullmatch(r"(\d+) checks, 0 mismatches\n", run.stdout)
    assert m and int(m.group(1)) == 736, run.stdout
    files = {}
    for name in FILES:
        with open(out / (name + ".parquet"), "rb") as f:
            files[name] = f.read()
    assert sorted(p.name for p in out.iterdir() if p.suffix == ".parquet") == sorted(n + ".parquet" for n in FILES)
    return files


# ---- the rules of tests/parquet_layout_main.cpp ---------------------------------------------------------------------------------
def rule_valid(r):
    return (r % 3 != 1) & ~((r >= 4096) & (r < 8192))


def rule_strings(r):
    return ["" if k % 7 == 3 else "".join(chr(97 + (k + i) % 26) for i in range((k * 5) % 23)) for k in r.tolist()]


def masked(values, valid, t):
    return pa.array(values, type=t, mask=~valid)


def rule_column(kind: int, rows: int):
    """(array, nullable, carries a bitmap) of column kind 0 .. 5"""
    r = np.arange(rows, dtype=np.int64)
    valid = rule_valid(r)
    flags = (r * 7) % 11 < 5
    if kind == 0:
        return pa.array((r.astype(np.uint64) * np.uint64(2654435761)).astype(np.uint32).view(np.int32)), False, False
    if kind == 1:
        return pa.array((r.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)).view(np.int64)), True, False
    if kind == 2:
        return masked(r * 0.5 - 1000.0, valid, pa.float64()), True, True
    if kind == 3:
        return masked(np.array(rule_strings(r), dtype=object), valid, pa.utf8()), True, True
    if kind == 4:
        return pa.array(flags), False, False
    return masked(flags, valid, pa.bool_()), True, True


SIX = ("req_i32", "opt_i64", "opt_f64", "s", "req_flag", "opt_flag")


def batch(columns):
    """columns: (name, array, nullable, bitmap) -> (record batch, names of the columns with a bitmap)"""
    rec = pa.RecordBatch.from_arrays([c[1] for c in columns], schema=pa.schema([pa.field(c[0], c[1].type, c[2]) for c in columns]))
    return rec, {c[0] for c in columns if c[3]}


def six(rows: int):
    return batch([(SIX[k], *rule_column(k, rows)) for k in range(6)])


# ---- reading a file three ways ----------------------------------------------------------------------------------------------------
def expected_bounds(col: pa.Array):
    """(min, max) the chunk must record, or None: NaNs and nulls take no part, a zero minimum is -0.0, a zero maximum +0.0,
    strings order as unsigned bytes, a bound longer than 4096 bytes is left out"""
    vals = [v for v in col.to_pylist() if v is not None and v == v]
    if not vals:
        return None
    if pa.types.is_string(col.type):
        lo, hi = min(vals, key=lambda s: s.encode()), max(vals, key=lambda s: s.encode())
        return None if max(len(lo.encode()), len(hi.encode())) > 4096 else (lo, hi)
    lo, hi = min(vals), max(vals)
    if pa.types.is_floating(col.type):
        lo, hi = (-0.0 if lo == 0 else lo), (0.0 if hi == 0 else hi)
    return lo, hi


def same_value(a, b) -> bool:
    return type(a) is type(b) and a == b and (not isinstance(a, float) or np.signbit(a) == np.signbit(b))


def one_batch(t: pa.Table) -> pa.RecordBatch:
    t = t.combine_chunks()
    return t.to_batches()[0] if t.num_rows else pa.RecordBatch.from_arrays([pa.array([], type=f.type) for f in t.schema], schema=t.schema)


def check_file(raw: bytes, groups, page_rows: int = PAGE_ROWS):
    """`groups`: one (record batch, columns with a bitmap) per row group"""
    pf = pq.ParquetFile(io.BytesIO(raw))
    md = pf.metadata
    want_schema = groups[0][0].schema
    assert md.num_row_groups == len(groups) and md.num_rows == sum(g[0].num_rows for g in groups)
    assert md.created_by == "chapterhouseqe_amd (MI355X page encoder)"
    assert [(f.name, f.type, f.nullable) for f in pf.schema_arrow] == [(f.name, f.type, f.nullable) for f in want_schema]
    pages = U.unpage(raw)                      # (asserts sizes, value counts, and that pages and chunks tile [4, footer))
    rebuilt = U.reassemble(raw, pages)
    mine = chq.ParquetFile(raw)
    head, cols, rgs = parse(mine.describe())
    mine.close()
    assert (int(head["rows"]), int(head["row_groups"]), int(head["columns"])) == (md.num_rows, len(groups), len(want_schema))
    assert [(c[1], c[2], c[3]) for c in cols] == [(f.name, md.schema.column(i).physical_type, "optional" if f.nullable else "required")
                                                  for i, f in enumerate(want_schema)]
    assert [("utf8" in c) for c in cols] == [pa.types.is_string(f.type) for f in want_schema]
    at = 4
    for g, (want, bitmaps) in enumerate(groups):
        rows = want.num_rows
        rg = md.row_group(g)
        assert rg.num_rows == rows == rgs[g]["rows"]
        got = one_batch(pf.read_row_group(g))
        assert batches_identical(got, want), f"pyarrow, row group {g}:\n{explain_diff(got, want)}"
        assert batches_identical(rebuilt[g], want), f"the pages, row group {g}:\n{explain_diff(rebuilt[g], want)}"
        n_pages = max(1, -(-rows // page_rows))
        for ci, f in enumerate(want_schema):
            col, cm, ch = want.column(ci), rg.column(ci), rgs[g]["chunks"][ci]
            # chunk offsets and lengths tile the body
            assert cm.data_page_offset == cm.file_offset == at and not cm.has_dictionary_page, (g, f.name)
            assert cm.total_compressed_size == cm.total_uncompressed_size > 0, (g, f.name)
            if rows:            # (the library's reader does not walk the pages of a chunk without values)
                assert cm.total_compressed_size == sum(p["bytes"] + p["header"] for p in ch["pages"]), (g, f.name)
            at += cm.total_compressed_size
            assert cm.num_values == rows == ch["values"] and cm.compression == "UNCOMPRESSED" and ch["codec"] == 0, (g, f.name)
            assert set(cm.encodings) == {"PLAIN", "RLE"}, (g, f.name)
            # statistics
            st = cm.statistics
            assert st is not None and st.has_null_count and st.null_count == col.null_count, (g, f.name)
            bounds = expected_bounds(col)
            assert st.has_min_max == (bounds is not None), (g, f.name)
            if bounds:
                assert same_value(st.min, bounds[0]) and same_value(st.max, bounds[1]), (g, f.name, st.min, st.max, bounds)
            # pages: page k holds rows [k * page_rows, (k + 1) * page_rows); a Boolean column with a bitmap is one page
            ps = [p for p in pages if (p.row_group, p.column) == (g, ci)]
            one_page = pa.types.is_boolean(f.type) and f.name in bitmaps
            assert len(ps) == (1 if one_page else n_pages) and len(ch["pages"]) == (len(ps) if rows else 0), (g, f.name, len(ps), n_pages)
            for k, p in enumerate(ps):
                r0, r1 = (0, rows) if one_page else (k * page_rows, min(rows, (k + 1) * page_rows))
                assert p.num_values == r1 - r0 and (not rows or ch["pages"][k]["values"] == r1 - r0), (g, f.name, k)
                assert arrays_identical(U.page_array(p), col.slice(r0, r1 - r0)), f"{f.name}: page {k} does not hold rows [{r0}, {r1})"
                assert p.optional == f.nullable and (p.level_bytes > 0) == f.nullable, (g, f.name, k)
                if f.nullable and f.name not in bitmaps:      # one RLE run: a length prefix, a varint, the level (no rows: no run)
                    assert p.level_bytes == (4 + len(varint(2 * p.num_values)) + 1 if p.num_values else 4), (g, f.name, k)
                if f.name in bitmaps and rows:
                    assert p.level_bytes == 4 + len(varint(2 * (-(-p.num_values // 8)) + 1)) + -(-p.num_values // 8), (g, f.name, k)
        assert rg.total_byte_size == sum(rg.column(ci).total_compressed_size for ci in range(rg.num_columns)), g
    flen = int.from_bytes(raw[-8:-4], "little")
    assert at == len(raw) - 8 - flen
    return pages


def varint(v: int) -> bytes:
    out = bytearray()
    while v >= 0x80:
        out.append(v & 0x7F | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", CUT_ROWS)
def test_page_cuts(written, rows):
    """required Int32 (cut by width), optional Int64 without a bitmap (RLE run), optional Float64 and Utf8 with nulls (cut by
    the block prefix; rows [4096, 8192) are all null), required Boolean (cut at bytes), nullable Boolean with nulls (one page)"""
    want, bitmaps = six(rows)
    pages = check_file(written["cuts_%d" % rows], [(want, bitmaps if rows else set())])
    if rows == 3 * 4096 + 5:
        for ci in (2, 3):       # the page whose every row is null: levels, no values
            p = [p for p in pages if p.column == ci][1]
            assert p.value_bytes == 0 and not p.levels.any() and p.end - p.payload_at == p.level_bytes


def test_a_chunk_is_widened_to_at_most_64_pages(written):
    rows = 64 * 4096 + 1
    col, nullable, _ = rule_column(0, rows)
    pages = check_file(written["widened"], [batch([(SIX[0], col, nullable, False)])], page_rows=8192)
    assert len(pages) == 33 and [p.num_values for p in pages] == [8192] * 32 + [1]


@pytest.mark.parametrize("name", ["page_rows_1", "page_rows_5000"])
def test_page_rows_round_down_to_a_multiple_of_4096(written, name):
    pages = check_file(written[name], [six(4097)])
    assert [p.num_values for p in pages if p.column == 0] == [4096, 1]
    assert written[name] == written["cuts_4097"]


def test_row_groups_tile_the_body(written):
    groups = [six(n) for n in ROW_GROUP_ROWS]
    groups[1] = (groups[1][0], set())          # (no rows: no bitmap)
    check_file(written["row_groups"], groups)
    got = one_batch(pq.read_table(io.BytesIO(written["row_groups"])))
    want = one_batch(pa.Table.from_batches([g[0] for g in groups]))
    assert batches_identical(got, want), explain_diff(got, want)


def test_thrift_long_list_and_two_byte_lengths(written):
    """lists of 15, 16 and 17 elements (the long list header), names of 130 and 131 bytes and a min_value of 4096 bytes (lengths
    as two-byte varints)"""
    for n in (15, 16):          # (a list of 15 elements is the first that needs the long header)
        check_file(written["schema_%d" % n], [batch([("c%d" % (10 + k), *rule_column(k % 6, 5)) for k in range(n)])])
    check_file(written["long_name"], [batch([("n" * 130, *rule_column(0, 5)), ("m" * 129 + "é", *rule_column(3, 5))])])
    lo = "".join(chr(97 + i % 26) for i in range(4096))
    check_file(written["long_bound"], [batch([("s", pa.array([lo, "b", "c"]), True, False)])])
    st = pq.ParquetFile(io.BytesIO(written["long_bound"])).metadata.row_group(0).column(0).statistics
    assert (st.min, st.max) == (lo, "c")


def test_statistics_bytes(written):
    """Int32 / Int64 extremes, float keys of +0.0 and -0.0 as minimum and as maximum, infinities, smallest subnormals, NaNs,
    Boolean, all-null columns (zero rows: test_page_cuts[0])"""
    nan, inf = float("nan"), float("inf")
    i32, i64 = np.iinfo(np.int32), np.iinfo(np.int64)
    tiny32, tiny64 = float(np.float32(1e-45)), 5e-324
    none4 = [None] * 4
    cases = [
        ("i32_extremes", pa.int32(), [i32.min, i32.max, 0, -1], (i32.min, i32.max)),
        ("i64_extremes", pa.int64(), [i64.max, i64.min, 0, -1], (i64.min, i64.max)),
        ("i32_only_min", pa.int32(), [i32.min] * 4, (i32.min, i32.min)),
        ("i64_only_max", pa.int64(), [i64.max] * 4, (i64.max, i64.max)),
    ]
    for nm, t, tiny in (("f32", pa.float32(), tiny32), ("f64", pa.float64(), tiny64)):
        cases += [
            (nm + "_pos_zero_min", t, [0.0, 1.0, 2.0, 1.0], (-0.0, 2.0)),
            (nm + "_neg_zero_min", t, [-0.0, 1.0, 2.0, 1.0], (-0.0, 2.0)),
            (nm + "_pos_zero_max", t, [0.0, -1.0, -2.0, -1.0], (-2.0, 0.0)),
            (nm + "_neg_zero_max", t, [-0.0, -1.0, -2.0, -1.0], (-2.0, 0.0)),
            (nm + "_both_zeros", t, [-0.0, 0.0, -0.0, 0.0], (-0.0, 0.0)),
            (nm + "_infinities", t, [1.5, inf, -inf, -2.5], (-inf, inf)),
            (nm + "_subnormals", t, [tiny, -tiny, 0.0, -0.0], (-tiny, tiny)),
        ]
    cases.insert(11, ("f32_nan_and_null", pa.float32(), [nan, 3.0, -nan, None], (3.0, 3.0)))
    cases += [
        ("f64_only_nans", pa.float64(), [nan, -nan, nan, nan], None),
        ("flag_mixed", pa.bool_(), [False, True, True, False], (False, True)),
        ("flag_all_false", pa.bool_(), [False] * 4, (False, False)),
        ("flag_all_true", pa.bool_(), [True] * 4, (True, True)),
        ("flag_true_under_null", pa.bool_(), [None, False, False, None], (False, False)),
        ("i32_all_null", pa.int32(), none4, None), ("f64_all_null", pa.float64(), none4, None),
        ("flag_all_null", pa.bool_(), none4, None), ("s_all_null", pa.utf8(), none4, None),
    ]
    want, bitmaps = batch([(nm, pa.array(v, type=t), True, None in v) for nm, t, v, _ in cases])
    check_file(written["statistics"], [(want, bitmaps)])
    rg = pq.ParquetFile(io.BytesIO(written["statistics"])).metadata.row_group(0)
    for ci, (nm, _t, v, bounds) in enumerate(cases):       # what the issue states outright, whatever expected_bounds() says
        st = rg.column(ci).statistics
        assert st.null_count == v.count(None) and st.has_min_max == (bounds is not None), nm
        if bounds:
            assert same_value(st.min, bounds[0]) and same_value(st.max, bounds[1]), (nm, st.min, st.max)
