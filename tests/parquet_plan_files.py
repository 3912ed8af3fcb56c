"""The files the Parquet scan's planning unit is checked on without a GPU (tests/test_parquet_scan_plan_host.py) and the scan
itself is compared on between two builds (profiles/parquet_scan_plan_refactor/compare.py): a pyarrow-written set over
required and optional columns of all six physical types, V1 and V2 pages, PLAIN and dictionary encodings, several pages a
chunk, an empty row group, uncompressed and snappy; every case of the two forged suites; and files with one defect the host
finds."""
import io

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq

from tests import parquet_forged_cases as F
from tests import snappy_forge as S
from tests import snappy_forged_cases as Z
from tests.parquet_cases import write_bytes

ROWS = 3000


def six_types(n: int, seed: int = 4) -> pa.Table:
    """a required and an optional column of every physical type the scan decodes"""
    rng = np.random.default_rng(seed)
    cols = {
        "flag": pa.array(rng.random(n) < 0.3), "i32": pa.array(rng.integers(-2**31, 2**31, n).astype(np.int32)),
        "i64": pa.array(rng.integers(-2**62, 2**62, n)), "f32": pa.array(rng.random(n).astype(np.float32)),
        "f64": pa.array(rng.standard_normal(n)), "s": pa.array(["w%d" % v * (v % 4) for v in rng.integers(0, 40, n)], type=pa.utf8()),
    }
    arrays, fields = [], []
    for name, a in cols.items():
        arrays.append(a)
        fields.append(pa.field("req_" + name, a.type, nullable=False))
        arrays.append(pa.array(a.to_pylist(), type=a.type, mask=rng.random(n) < 0.25))
        fields.append(pa.field("opt_" + name, a.type, nullable=True))
    return pa.table(arrays, schema=pa.schema(fields))


def with_empty_row_group(codec: str) -> bytes:
    t = six_types(700, seed=9)
    buf = io.BytesIO()
    with pq.ParquetWriter(buf, t.schema, compression=codec) as w:
        w.write_table(t.slice(0, 400))
        w.write_table(t.slice(0, 0))
        w.write_table(t.slice(400))
    raw = buf.getvalue()
    assert [pq.ParquetFile(io.BytesIO(raw)).metadata.row_group(g).num_rows for g in range(3)] == [400, 0, 300]
    return raw


def pyarrow_files() -> dict:
    out = {}
    t = six_types(ROWS)
    for codec in ("none", "snappy"):
        for ver in ("1.0", "2.0"):
            for dic in (True, False):
                for page in (1 << 20, 2000):          # (2000 bytes: several pages a chunk)
                    name = f"six_{codec}_v{ver[0]}_{'dict' if dic else 'plain'}_{page}"
                    out[name] = write_bytes(t, compression=codec, data_page_version=ver, use_dictionary=dic, data_page_size=page,
                                            write_batch_size=200, row_group_size=2000)
        out[f"empty_row_group_{codec}"] = with_empty_row_group(codec)
        out[f"no_statistics_{codec}"] = write_bytes(t, compression=codec, write_statistics=False, data_page_size=2000, write_batch_size=200)
    return out


def forged_files() -> dict:
    """name -> bytes of every case of tests/parquet_forged_cases.py and tests/snappy_forged_cases.py, the damaged ones too"""
    out = {}
    for name in F.CASES + F.BA_CASES + F.LENIENT + F.DAMAGED:
        out["forged " + name] = F.build(name).raw
    for name, make in F.PYARROW_FILES.items():
        for k, raw in enumerate(make()):
            out[f"forged {name} {k}"] = raw
    for name in list(Z.CASES) + list(Z.DAMAGED):
        out["snappy " + name] = Z.build(name).raw
    return out


DEVICE_DAMAGE = ["forged " + n for n in F.DAMAGED] + ["snappy " + n for n in Z.DAMAGED]


def levels_past_page(codec: str, row_groups: int = 2, rows: int = 300):
    """(table, bytes): an Int32 and a Utf8 column in `row_groups` row groups of V2 pages; the header of the LAST row group's
    first page of column `a` declares a level section of 1 MiB -- the footer and every page header parse, the scan's page loop
    refuses the page"""
    rng = np.random.default_rng(31)
    n = rows * row_groups
    t = pa.table({"a": pa.array(rng.integers(0, 1000, n).astype(np.int32)), "s": pa.array(["s%04d" % v for v in rng.integers(0, 9999, n)])})
    raw = write_bytes(t, compression=codec, row_group_size=rows, use_dictionary=False, data_page_version="2.0")
    hit = []

    def page_fn(info, payload):
        if (info.row_group, info.column, info.type) == (row_groups - 1, 0, S.DATA_PAGE_V2):
            info.header.get(8).set(5, 1 << 20)
            hit.append(info.page)
        return None
    bad = S.rewrite(raw, page_fn, None)
    assert hit == [0]
    return t, bad


LEVELS_PAST_PAGE = {"none": (22, "parquet: definition levels run past the page"), "snappy": (22, "parquet: level sections run past the page")}


def host_refused() -> dict:
    """name -> (bytes, code, text the message must hold): one defect each, found by the host before anything is launched"""
    t = six_types(100).select(["req_i32", "opt_s"])
    out = {}
    for codec, name in (("zstd", "ZSTD"), ("gzip", "GZIP"), ("lz4", "LZ4_RAW")):
        out["codec_" + codec] = (write_bytes(t, compression=codec), 30, f"parquet: compression codec {name} (column 'req_i32'); UNCOMPRESSED and SNAPPY pages are decoded")
    out["date32"] = (write_bytes(pa.table({"d": pa.array([1, 2, 3], type=pa.date32())})), 30, "parquet: logical type of column 'd'")
    out["delta_binary_packed"] = (write_bytes(pa.table({"v": pa.array(np.arange(1000, dtype=np.int64))}), use_dictionary=False,
                                              column_encoding={"v": "DELTA_BINARY_PACKED"}), 30, "parquet: encoding 5 (column 'v')")
    for codec in ("none", "snappy"):
        out["levels_past_page_" + codec] = (levels_past_page(codec)[1], *LEVELS_PAST_PAGE[codec])
    return out
