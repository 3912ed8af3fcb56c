"""GPU: the serial page decoders of csrc/parquet.hip -- hybrid_decode_block behind the level, dictionary-index and RLE-boolean
kernels, and the speculative PLAIN BYTE_ARRAY walk -- on streams no Arrow writer emits: bit-packed runs of thousands of
groups and of many LDS windows, bit widths 0 to 32, padded varints, runs and headers laid against the window end, cut-off
last groups, strings whose prefixes straddle the walk's window or whose bytes imitate prefixes.  Every file
(tests/parquet_forged_cases.py, whose builders assert the shapes against a model of the kernels' windows) is compared
bit-exact with pyarrow's reader on the same bytes; damage must be a ChqError that leaves the context usable."""
import pytest

import chapterhouseqe_amd as chq
from tests.parquet_forged_cases import BA_CASES, CASES, DAMAGED, HOST_RESULT, LENIENT, PYARROW_FILES, build, good_file
from tests.scan_compare import check

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = chq.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("name", CASES)
def test_forged_hybrid_streams_decode_like_pyarrow(ctx, name):
    """dictionary Int32 / Utf8 indices, definition levels and RLE booleans of the named shape, V1 / V2 pages, uncompressed
    and snappy (where V1 levels and values are told apart on the device)"""
    check(build(name).raw, ctx)


@pytest.mark.parametrize("name", HOST_RESULT)
def test_forged_hybrid_streams_into_a_host_result(ctx, name):
    check(build(name).raw, ctx, device_result=False)


@pytest.mark.parametrize("name", BA_CASES)
def test_plain_byte_array_pages_walk_like_pyarrow(ctx, name):
    """PLAIN strings laid against the walk's 32 KiB window, uniform runs broken at chosen lanes, imitated prefixes, bursts;
    as a data page and as the dictionary page of a snappy chunk (walked on the device)"""
    f = build(name)
    check(f.raw, ctx)
    if name.endswith("plain-v1-none"):
        check(f.raw, ctx, device_result=False)


@pytest.mark.parametrize("name", list(PYARROW_FILES))
def test_page_counts_and_empty_pages(ctx, name):
    """chunks of more than 256 pages, and pages without a value between pages that have some (files pyarrow writes)"""
    for raw in PYARROW_FILES[name]():
        check(raw, ctx)


@pytest.mark.parametrize("name", LENIENT)
def test_shapes_pyarrow_refuses_are_an_error_or_the_tolerant_values(ctx, name):
    """The three shapes pyarrow answers with "Unexpected end of stream".  The scan today: a run of zero repetitions and a
    bit-packed run of zero groups are skipped and the page decodes to the table's values, unless the zero-group run is the
    first thing of the stream's last window, where the stream counts as ended (a ChqError if values are still missing); a
    header that declares more groups than the stream holds yields the values the bytes hold, and a ChqError only if those
    are fewer than the page's.  The files here hold one window a stream, so by the kernel's rules the zero-group ones are a
    ChqError and the other two decode to their tables."""
    f = build(name)
    assert f.lenient
    try:
        check(f.raw, ctx, table=f.table)
    except chq.ChqError as e:
        assert e.code in (22, 30), str(e)
    check(good_file().raw, ctx)


@pytest.mark.parametrize("name", DAMAGED)
def test_damaged_streams_are_reported(ctx, name):
    """a stream that ends early or inside a header or an RLE value, a dictionary index beyond the dictionary, a bit width
    above 32, levels shorter than the rows, a length prefix past the page: a ChqError, never values; the same context then
    reads a valid file"""
    f = build(name)
    assert f.damaged
    pf = chq.ParquetFile(f.raw)
    with pytest.raises(chq.ChqError) as e:
        pf.read_row_group(0, ctx=ctx)
    assert e.value.code in (22, 30), str(e.value)
    pf.close()
    check(good_file().raw, ctx)
