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
    # the one geometry (scan_device.h): a tile is a workgroup's threads times their items
    shared = source("scan_device.h")
    block, items = constant(shared, "kScanBlock"), constant(shared, "kScanItems")
    assert re.search(r"constexpr\s+int\s+kScanTile\s*=\s*kScanBlock\s*\*\s*kScanItems\s*;", shared)
    assert G.T == block * items

    # every operator's constants are tied to it: a static_assert in its kernels, an alias of the aggregate's for join and window
    agg, part, sort, strfn, join, win = (source(h) for h in ("aggregate_device.h", "partition_device.h", "sort_device.h", "strfn_device.h",
                                                             "join_device.h", "window_device.h"))
    for name, header, kernels in (("Agg", agg, "aggregate.hip"), ("Part", part, "partition.hip"), ("Sort", sort, "sort.hip")):
        assert constant(header, f"k{name}Block") == block and constant(header, f"k{name}Items") == items, name
        assert re.search(rf"constexpr\s+int\s+k{name}Tile\s*=\s*k{name}Block\s*\*\s*k{name}Items\s*;", header), name
        assert f"static_assert(k{name}Block == kScanBlock && k{name}Items == kScanItems && k{name}Tile == kScanTile," in source(kernels), name
    for name in ("Block", "Items", "Tile"):
        assert re.search(rf"constexpr\s+int\s+kJoin{name}\s*=\s*kAgg{name}\s*;", join), name
        assert re.search(rf"constexpr\s+int\s+kWin{name}\s*=\s*kAgg{name}\s*;", win), name
    scan = source("scan.hip")
    assert "static_assert(kJoinTile == kScanTile && STRFN_SCAN_CHUNK == kScanTile," in scan
    assert G.T == constant(strfn, "STRFN_SCAN_CHUNK")

    # scan_totals_in_place, the one loop over tile totals: one total per thread of ONE workgroup and round.  Its three users --
    # the offsets scan of the join and the string functions, the Utf8 gather of the sort, the group heads -- launch it alike.
    loop = body_of(shared, "void scan_totals_in_place(")
    assert only(r"c0 \+= (\w+)\)", loop) == "kScanBlock" and "t = c0 + threadIdx.x;" in loop
    assert len(re.findall(r"c0 \+= ", shared)) == 2                            # (the other one: scan_count_rows, below)
    for text, kernel, name in ((scan, "scan_totals_kernel", "Scan"), (source("sort.hip"), "sort_utf8_scan_sums_kernel", "Sort"),
                               (source("aggregate.hip"), "agg_head_scan_kernel", "Agg")):
        assert "scan_totals_in_place<" in body_of(text, f"void {kernel}("), kernel
        assert f"{kernel}, dim3(1), dim3(k{name}Block)" in text, kernel
    assert "launch_offsets_scan(" in source("join.cpp")
    assert source("materialize.cpp").count("launch_offsets_scan(") == 1   # (the one Utf8 assembly of the string functions, CASE and CAST)
    assert G.SCAN_ROUND == G.STRFN_ROUND == block * G.T

    # ... and the three scans of the Parquet kernels: the same loop over page counts and over the totals of blocks of
    # PQ_SCAN_ROWS / PW_BLOCK_ROWS rows, which parquet_device.h defines once for the host (n_blocks) and the kernels
    shared_pq = source("parquet_device.h")
    assert G.PQ_BLOCK == constant(shared_pq, "PQ_SCAN_ROWS") == constant(shared_pq, "PW_BLOCK_ROWS")
    for name, kernels in (("PQ_SCAN_ROWS", ("parquet.hip", "parquet_scan.cpp")), ("PW_BLOCK_ROWS", ("parquet_write.hip", "parquet_write.cpp"))):
        for text in map(source, kernels):
            assert name in text and not re.search(r"constexpr\s+int\s+" + name, text), name
    pq, pw = source("parquet.hip"), source("parquet_write.hip")
    for text, kernel, total in ((pq, "pq_page_scan_kernel", "p.total_values"), (pq, "pq_rowlen_scan_kernel", "p.total_bytes"),
                                (pw, "pw_scan_kernel", "p.total_bytes")):
        assert "scan_totals_in_place<" in body_of(text, f"void {kernel}(") and f", {total}, sums);" in body_of(text, f"void {kernel}("), kernel
        assert f"{kernel}, dim3(1), dim3(kScanBlock)" in text, kernel
    assert "(int64_t)blockIdx.x * PQ_SCAN_ROWS" in body_of(pq, "void pq_rowlen_sums_kernel(")
    assert "(int64_t)blockIdx.x * PW_BLOCK_ROWS" in body_of(pw, "void pw_counts_kernel(")
    assert G.PQ_ROUND == block * G.PQ_BLOCK and G.PQ_ROWS == G.PQ_ROUND + 1

    # part_scan_kernel (and sort_scan_kernel): scan_count_rows with kPartItems tile counts per thread and round, a round of
    # kPartTile counts
    loop = body_of(shared, "void scan_count_rows(")
    assert only(r"c0 \+= ([\w *]+)\)", loop) == "kScanBlock * ITEMS" and "threadIdx.x * ITEMS" in loop
    text = source("partition.hip")
    assert "scan_count_rows<kPartItems>(" in body_of(text, "void part_scan_kernel(")
    assert "part_scan_kernel, dim3(p.n_partitions), dim3(kPartBlock)" in text
    assert "scan_count_rows<kSortItems>(" in body_of(source("sort.hip"), "void sort_scan_kernel(")
    assert G.PART_ROUND == (block * items) * G.T
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
