"""GPU: the snappy inflate kernels (csrc/parquet_codec.hip) on forged streams of every legal shape -- copy-4 tags, offsets
around and beyond the 64 KiB LDS ring up to 1 MiB, copies of length 1 to 3, every literal header width, elements across
64 KiB output blocks, copies into the previous block, segment bounds on and inside element headers, guesses that cannot
meet the chain, padded preambles, V2 sections stored or empty, forged dictionary pages -- which Google's compressor never
writes.  Each file (tests/snappy_forged_cases.py, whose builders assert the shapes) is read on four contexts, one per
value of option snappy_blocks, so every inflate path decodes the same bytes, and compared bit-exact with pyarrow's reader.
Damaged streams must be reported as ChqError and leave the context usable."""
import io

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

import chapterhouseqe_amd as chq
from tests.snappy_forged_cases import CASES, DAMAGED, MODES, build

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def contexts():
    cs = {}
    for m in MODES:
        cs[m] = chq.Context(0)
        if m != 1:
            cs[m].set_option("snappy_blocks", m)
    yield cs
    for c in cs.values():
        c.close()


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
    else:
        width = w.type.bit_width // 8
        xv = np.frombuffer(x.buffers()[1], dtype=np.uint8)[x.offset * width:(x.offset + len(x)) * width].reshape(-1, width)
        wv = np.frombuffer(w.buffers()[1], dtype=np.uint8)[w.offset * width:(w.offset + len(w)) * width].reshape(-1, width)
        assert (xv[valid] == wv[valid]).all(), f"{what}: values"
    assert x.equals(w), what


def check(raw: bytes, ctx):
    exp = pq.ParquetFile(io.BytesIO(raw))
    f = chq.ParquetFile(raw)
    assert f.num_row_groups == exp.metadata.num_row_groups
    for g in range(f.num_row_groups):
        want = exp.read_row_group(g).combine_chunks()
        got = f.read_row_group(g, ctx=ctx).to_host()
        assert got.num_rows == want.num_rows and got.schema.names == want.schema.names
        for i, name in enumerate(want.schema.names):
            w = want.column(i).chunk(0) if want.num_rows else pa.array([], type=want.schema.field(i).type)
            same_bits(got.column(i), w, f"{name}: row group {g}")
    f.close()


@pytest.mark.parametrize("name", list(CASES))
def test_forged_snappy_pages_decode_like_pyarrow(contexts, name):
    """the case's page through every inflate path: one wave per page (snappy_blocks 0), block by block after an INDEX or
    segmented walk (1, the default), with the FINISH redo forced (2), with the walk never segmented (3)"""
    f = build(name)
    for m in MODES:
        check(f.raw, contexts[m])


@pytest.mark.parametrize("name", list(DAMAGED))
def test_damaged_forged_snappy_pages_are_reported(contexts, name):
    """damage the format forbids is a ChqError on every path, never values; the same context then reads a valid file"""
    f = build(name)
    assert f.damaged
    good = build("far_offsets_one_wave")
    for m in MODES:
        pf = chq.ParquetFile(f.raw)
        with pytest.raises(chq.ChqError) as e:
            pf.read_row_group(0, ctx=contexts[m])
        assert e.value.code in (22, 30), str(e.value)
        pf.close()
        check(good.raw, contexts[m])
