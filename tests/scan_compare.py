"""The comparison of a Parquet scan with pyarrow's reader that the forged-file GPU tests share."""
import io

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq

import chapterhouseqe_amd as chq


def same_bits(x: pa.Array, w: pa.Array, what: str):
    """bit-exact: validity, null count, and every buffer's defined bytes (Utf8: offsets and string bytes)"""
    assert x.type == w.type and len(x) == len(w) and x.null_count == w.null_count, what
    valid = np.ones(len(w), dtype=bool) if w.null_count == 0 else ~np.asarray(w.is_null())
    if x.null_count:
        assert (~np.asarray(x.is_null()) == valid).all(), what
    if pa.types.is_string(w.type):
        xo = np.frombuffer(x.buffers()[1], dtype=np.int32)[x.offset:x.offset + len(x) + 1]
        wo = np.frombuffer(w.buffers()[1], dtype=np.int32)[w.offset:w.offset + len(w) + 1]
        assert ((xo - xo[0]) == (wo - wo[0])).all(), f"{what}: offsets"
        xd, wd = x.buffers()[2], w.buffers()[2]
        assert (xd.to_pybytes()[xo[0]:xo[-1]] if xd else b"") == (wd.to_pybytes()[wo[0]:wo[-1]] if wd else b""), f"{what}: bytes"
    elif pa.types.is_boolean(w.type):
        xb = np.unpackbits(np.frombuffer(x.buffers()[1], dtype=np.uint8), bitorder="little")[x.offset:x.offset + len(x)]
        wb = np.unpackbits(np.frombuffer(w.buffers()[1], dtype=np.uint8), bitorder="little")[w.offset:w.offset + len(w)]
        assert (xb[valid] == wb[valid]).all(), f"{what}: values"
    else:
        width = w.type.bit_width // 8
        xv = np.frombuffer(x.buffers()[1], dtype=np.uint8)[x.offset * width:(x.offset + len(x)) * width].reshape(-1, width)
        wv = np.frombuffer(w.buffers()[1], dtype=np.uint8)[w.offset * width:(w.offset + len(w)) * width].reshape(-1, width)
        assert (xv[valid] == wv[valid]).all(), f"{what}: values"
    assert x.equals(w), what


def check(raw: bytes, ctx, device_result: bool = True, table: pa.Table = None):
    """every row group of `raw` as the scan reads it against pyarrow's reader on the same bytes (`table`: against this
    table instead, for one-row-group files pyarrow refuses)"""
    exp = pq.ParquetFile(io.BytesIO(raw))
    f = chq.ParquetFile(raw)
    assert f.num_row_groups == exp.metadata.num_row_groups and (table is None or f.num_row_groups == 1)
    for g in range(f.num_row_groups):
        want = (exp.read_row_group(g) if table is None else table).combine_chunks()
        got = f.read_row_group(g, ctx=ctx, device_result=device_result)
        if device_result:
            got = got.to_host()
        assert got.num_rows == want.num_rows and got.schema.names == want.schema.names
        for i, name in enumerate(want.schema.names):
            w = want.column(i).chunk(0) if want.num_rows else pa.array([], type=want.schema.field(i).type)
            same_bits(got.column(i), w, f"{name}: row group {g}")
    f.close()
