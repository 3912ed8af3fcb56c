"""Host: the round sizes that tests/test_gpu_rounds.py hard-codes against the tiles, scan rounds and grid caps of the sources.
If a tile or a cap is retuned, the GPU tests would silently stop reaching the second round of the loops they are there for;
this test fails instead.  Plain text matching on the project's own headers and kernels, nothing more."""
import os
import re

from . import test_gpu_rounds as G

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "chapterhouseqe_amd", "csrc")


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def constant(text, name):
    """`constexpr int NAME = <integer>;`"""
    found = re.findall(r"constexpr\s+int\s+" + name + r"\s*=\s*(\d+)\s*;", text)
    assert len(found) == 1, (name, found)
    return int(found[0])


def product(expr):
    """`256 * 32` -> 8192"""
    out = 1
    for factor in expr.split("*"):
        out *= int(factor)
    return out


def body_of(text, head):
    """the text from the one line that holds `head` to the next line that is a lone closing brace"""
    assert text.count(head) == 1, (head, text.count(head))
    start = text.index(head)
    return text[start:text.index("\n}", start)]


def only(pattern, text):
    found = re.findall(pattern, text)
    assert len(found) == 1, (pattern, found)
    return found[0]


def test_tiles_of_the_scans():
    agg, part, sort, strfn, join = (source(h) for h in ("aggregate_device.h", "partition_device.h", "sort_device.h", "strfn_device.h", "join_device.h"))
    agg_block, agg_items = constant(agg, "kAggBlock"), constant(agg, "kAggItems")
    part_block, part_items = constant(part, "kPartBlock"), constant(part, "kPartItems")
    sort_block, sort_items = constant(sort, "kSortBlock"), constant(sort, "kSortItems")
    for name, of in (("Agg", agg), ("Part", part), ("Sort", sort)):           # a tile is a workgroup's threads times their items
        assert re.search(rf"constexpr\s+int\s+k{name}Tile\s*=\s*k{name}Block\s*\*\s*k{name}Items\s*;", of), name
    for name in ("Block", "Items", "Tile"):                                    # the join kernels take the aggregate's geometry
        assert re.search(rf"constexpr\s+int\s+kJoin{name}\s*=\s*kAgg{name}\s*;", join), name
    assert G.T == agg_block * agg_items == part_block * part_items == sort_block * sort_items == constant(strfn, "STRFN_SCAN_CHUNK")

    # join_scan_sums_kernel, sort_utf8_scan_sums_kernel: one tile total per thread of ONE workgroup and round
    scan = body_of(source("join.hip"), "void join_scan_sums_kernel(")
    assert only(r"c0 \+= (\w+)\)", scan) == "kJoinBlock" and "dim3(1), dim3(kJoinBlock)" in body_of(source("join.hip"), "hipError_t launch_join_scan(")
    assert G.SCAN_ROUND == agg_block * G.T
    scan = body_of(source("sort.hip"), "void sort_utf8_scan_sums_kernel(")
    assert only(r"c0 \+= (\w+)\)", scan) == "kSortBlock"
    assert "sort_utf8_scan_sums_kernel, dim3(1), dim3(kSortBlock)" in source("sort.hip")
    assert G.SCAN_ROUND == sort_block * G.T

    # part_scan_kernel: kPartItems tile counts per thread and round
    scan = body_of(source("partition.hip"), "void part_scan_kernel(")
    assert only(r"c0 \+= (\w+)\)", scan) == "kPartTile" and "threadIdx.x * kPartItems" in scan
    assert "part_scan_kernel, dim3(p.n_partitions), dim3(kPartBlock)" in source("partition.hip")
    assert G.PART_ROUND == (part_block * part_items) * G.T

    # strfn_scan_chunks_kernel: one wave, one chunk total per lane and round
    text = source("strfn.hip")
    scan = body_of(text, "void strfn_scan_chunks_kernel(")
    lanes = int(only(r"c0 \+= (\d+)\)", scan))
    assert lanes == 64 and f"strfn_scan_chunks_kernel, dim3(1), dim3({lanes})" in text
    assert G.STRFN_ROUND == lanes * constant(source("strfn_device.h"), "STRFN_SCAN_CHUNK")
    assert G.SCAN_ROWS == G.SCAN_ROUND + G.T + 5 and G.PART_ROWS == G.PART_ROUND + G.T + 5 and G.STRFN_ROWS == G.STRFN_ROUND + G.T + 5


def test_caps_of_the_strided_grids():
    # typed_ops.hip: grid_for caps every launch of the file at 256 * 32 workgroups of 256 threads
    text = source("typed_ops.hip")
    cap = only(r"blocks > (\d+ \* \d+) \? (\d+ \* \d+) : blocks", body_of(text, "static int grid_for("))
    assert product(cap[0]) == product(cap[1]) and G.STRIDE_ROWS == product(cap[0]) * 256
    for kernel in ("cmp128_kernel", "is_null_kernel", "utf8_to_bool_kernel", "utf8_uniform_kernel"):
        assert f"{kernel}, dim3(grid_for(p.nrows)), dim3(256)" in text, kernel
        assert "+= (int64_t)gridDim.x * 256" in body_of(text, f"void {kernel}("), kernel
    assert "iota_offsets_kernel, dim3(grid_for(p.n_plus_1)), dim3(256)" in text

    # like.hip: the same cap, spelled out in launch_like
    text = source("like.hip")
    cap = only(r"blocks > (\d+ \* \d+) \? (\d+ \* \d+) : blocks\)\), dim3\(256\)", body_of(text, "hipError_t launch_like("))
    assert product(cap[0]) == product(cap[1]) and G.STRIDE_ROWS == product(cap[0]) * 256
    assert "+= (int64_t)gridDim.x * 256" in body_of(text, "void like_kernel(")

    # strfn.hip: capped_grid(items, cap) workgroups of 256 threads; the byte map takes 16 bytes per thread
    text = source("strfn.hip")
    caps = {kernel: (items, product(cap)) for kernel, items, cap in
            re.findall(r"hipLaunchKernelGGL\((\w+), dim3\(capped_grid\(([^,]+), (\d+ \* \d+)\)\), dim3\(256\)", text)}
    assert sorted(caps) == ["strfn_bytemap_kernel", "strfn_gather_kernel", "strfn_rebase_kernel", "strfn_rows_kernel"], caps
    assert caps["strfn_rows_kernel"] == ("p.nrows", G.STRIDE_ROWS // 256) and caps["strfn_gather_kernel"] == ("p.nrows", G.STRIDE_ROWS // 256)
    assert caps["strfn_rebase_kernel"] == ("p.n", G.REBASE_ROWS // 256)
    assert caps["strfn_bytemap_kernel"] == ("p.n / 16 + 1", G.BYTEMAP_BYTES // (256 * 16))
    assert "nvec = (p.n - head) >> 4" in body_of(text, "void strfn_bytemap_kernel(")
    assert G.STRIDE_N == G.STRIDE_ROWS + 64 + 1 and G.STRIDE_N > G.REBASE_ROWS and G.STRIDE_N * 9 * 0.9 > G.BYTEMAP_BYTES   # (9-byte rows, a tenth of them null)
