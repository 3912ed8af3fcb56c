"""GPU: the snappy inflate kernels (csrc/parquet_codec.hip) on forged streams of every legal shape -- copy-4 tags, offsets
around and beyond the 64 KiB LDS ring up to 1 MiB, copies of length 1 to 3, every literal header width, elements across
64 KiB output blocks, copies into the previous block, segment bounds on and inside element headers, guesses that cannot
meet the chain, padded preambles, V2 sections stored or empty, forged dictionary pages -- which Google's compressor never
writes.  Each file (tests/snappy_forged_cases.py, whose builders assert the shapes) is read on four contexts, one per
value of option snappy_blocks, so every inflate path decodes the same bytes, and compared bit-exact with pyarrow's reader.
Damaged streams must be reported as ChqError and leave the context usable."""
import pytest

import chapterhouseqe_amd as chq
from tests.scan_compare import check
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
