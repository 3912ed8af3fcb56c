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


# the twelve kernels on the row loop of wave_rows.h (a wave per 64 rows, rounds of the launched grid) ...
ROW_KERNELS = {"typed_ops.hip": ("cmp128_kernel", "utf8_to_bool_kernel", "is_null_kernel"),
               "like.hip": ("like_kernel",),
               "strfn.hip": ("strfn_rows_kernel", "strfn_gather_kernel"),
               "case.hip": ("case_select_fixed_kernel", "case_rows_kernel", "case_gather_kernel"),
               "cast.hip": ("cast_fixed_kernel", "cast_parse_kernel", "cast_len_kernel")}
# ... and every launch of the five files: kernel -> (items, cap in workgroups).  The one launch that is not rows_grid's:
TWO_DIMENSIONAL = "utf8_uniform_group_kernel"   # grid = (batches, slices of a batch), both sized in launch_utf8_uniform_group
LAUNCHES = {
    "typed_ops.hip": {"cmp128_kernel": ("p.nrows", "256 * 32"), "is_null_kernel": ("p.nrows", "256 * 32"), "utf8_uniform_kernel": ("p.nrows", "256 * 32"),
                      "iota_offsets_kernel": ("p.n_plus_1", "256 * 32"), "utf8_to_bool_kernel": ("p.nrows", "256 * 32"), TWO_DIMENSIONAL: None},
    "like.hip": {"like_kernel": ("p.nrows", "256 * 32")},
    "strfn.hip": {"strfn_bytemap_kernel": ("p.n / 16 + 1", "256 * 16"), "strfn_rebase_kernel": ("p.n", "256 * 16"),
                  "strfn_rows_kernel": ("p.nrows", "256 * 32"), "strfn_gather_kernel": ("p.nrows", "256 * 32")},
    "case.hip": {"case_masks_kernel": ("p.words", "256 * 32"), "case_and_kernel": ("(p.nrows + 63) / 64", "256 * 32"),
                 "case_select_bool_kernel": ("p.words", "256 * 32"), "case_select_fixed_kernel": ("p.nrows", "256 * 32"),
                 "case_rows_kernel": ("p.nrows", "256 * 32"), "case_gather_kernel": ("p.nrows", "256 * 32")},
    "cast.hip": {"cast_fixed_kernel": ("p.nrows", "CAST_GRID_CAP"), "cast_parse_kernel": ("p.nrows", "CAST_GRID_CAP"),
                 "cast_len_kernel": ("p.nrows", "CAST_GRID_CAP"), "cast_write_kernel": ("p.nrows", "CAST_GRID_CAP")},
}


def test_caps_of_the_strided_grids():
    # the round loop is written once, in wave_rows.h (a loop-head macro), and strides by the launched grid of kRowsBlock threads
    every = {name: source(name) for name in sorted(os.listdir(CSRC)) if name.endswith((".hip", ".h")) and name != "kernels.hip"}
    head = r"for \(int64_t base = \(\(int64_t\)blockIdx\.x \* (\w+) \+ threadIdx\.x\) & ~63LL; base < ([\w.()]+); base \+= \(int64_t\)gridDim\.x \* (\w+)\)"
    assert [(name, found) for name, text in every.items() for found in re.findall(head, text)] == [("wave_rows.h", ("kRowsBlock", "(nrows)", "kRowsBlock"))]
    assert sum(text.count("& ~63LL") for text in every.values()) == 1
    rows = every["wave_rows.h"]
    block = constant(rows, "kRowsBlock")
    assert re.search(r"#define CHQ_FOR_WAVE_ROWS\(base, nrows\) \\\n  for \(int64_t base = [^\n]*& ~63LL;", rows)
    assert sum(text.count("#define CHQ_FOR_WAVE_ROWS") for text in every.values()) == 1
    cast_block = constant(every["cast_device.h"], "CAST_BLOCK")
    assert "static_assert(CAST_BLOCK == kRowsBlock," in every["cast.hip"] and cast_block == block
    for name, kernels in ROW_KERNELS.items():
        for kernel in kernels:
            body = body_of(every[name], f"void {kernel}(")
            assert body.count("CHQ_FOR_WAVE_ROWS(base, p.nrows) {\n    const int64_t i = base + lane_id()") == 1 == body.count("CHQ_FOR_WAVE_ROWS"), kernel
            assert "blockIdx" not in body and "gridDim" not in body and body.endswith("\n  }"), kernel   # (no loop of its own around or behind it)
            assert re.search(r"__launch_bounds__\((kRowsBlock|CAST_BLOCK)\) void " + kernel + r"\(", every[name]), kernel
    assert sum(len(kernels) for kernels in ROW_KERNELS.values()) == 12 == sum(text.count("CHQ_FOR_WAVE_ROWS(base, p.nrows)") for text in every.values())

    # the clamp is written once, in rows_grid: ceil(items / kRowsBlock) workgroups, at least 1, at most the cap the launch names
    clamp = "blocks < 1 ? 1 : blocks > cap_blocks ? cap_blocks : blocks"
    grid = body_of(every["typed_ops.h"], "inline unsigned rows_grid(int64_t items, int64_t cap_blocks) {")
    assert f"return (unsigned)({clamp});" in grid and f"blocks = (items + {block - 1}) / {block};" in grid
    assert sum(text.count(clamp) for text in every.values()) == 1
    code = lambda text: re.sub(r"//[^\n]*", "", text)
    assert sum(len(re.findall(r"blocks\s*>", code(text))) for name, text in every.items() if name in LAUNCHES or name == "typed_ops.h") == 1
    # (case.hip's head comment quotes the clamp with its cap for tests/test_gpu_case.py: held to the launches below)
    assert only(r"// .*`blocks > (\d+ \* \d+) \? \1 : blocks`", every["case.hip"]) == LAUNCHES["case.hip"]["case_rows_kernel"][1]

    # every launch of the five files takes its grid from it, with its cap spelled at the call, and workgroups of kRowsBlock threads
    caps = {}
    for name, expected in LAUNCHES.items():
        text = every[name]
        launches = re.findall(r"hipLaunchKernelGGL\(\(?(\w+)(?:<[\w, ]+>)?\)?, (dim3\(.+?\)|grid), (dim3\(\w+\)|block), 0, stream, p\)", text)
        assert len(launches) == text.count("hipLaunchKernelGGL(") and {kernel for kernel, _, _ in launches} == set(expected), (name, launches)
        for kernel, grid, threads in launches:
            if grid == "grid":    # (one dim3 for the instantiations of a template)
                grid, threads = only(r"const dim3 grid\((rows_grid\(.+?\))\), block\((\w+)\);", text)
                grid, threads = f"dim3({grid})", f"dim3({threads})"
            assert threads in ("dim3(256)", "dim3(CAST_BLOCK)", "dim3(kRowsBlock)") and block == 256, (kernel, threads)
            if kernel == TWO_DIMENSIONAL:
                assert grid == "dim3(gx, (unsigned)gy)"
                continue
            items, cap = expected[kernel]
            assert grid == f"dim3(rows_grid({items}, {cap}))", (kernel, grid)
            if cap != "CAST_GRID_CAP":   # (tests/test_cast_host.py holds that one to the sizes of the cast tests)
                caps[kernel] = product(cap)

    # the sizes of tests/test_gpu_rounds.py against those caps; the plain grid-stride loops step by the same 256 threads
    for kernel in ("cmp128_kernel", "is_null_kernel", "utf8_to_bool_kernel", "utf8_uniform_kernel", "like_kernel", "strfn_rows_kernel", "strfn_gather_kernel"):
        assert G.STRIDE_ROWS == caps[kernel] * block, kernel
    assert "+= (int64_t)gridDim.x * 256" in body_of(every["typed_ops.hip"], "void utf8_uniform_kernel(")
    assert G.REBASE_ROWS == caps["strfn_rebase_kernel"] * block and "+= (int64_t)gridDim.x * 256" in body_of(every["strfn.hip"], "void strfn_rebase_kernel(")
    assert G.BYTEMAP_BYTES == caps["strfn_bytemap_kernel"] * block * 16   # (the byte map takes 16 bytes per thread)
    assert "nvec = (p.n - head) >> 4" in body_of(every["strfn.hip"], "void strfn_bytemap_kernel(")
    assert G.STRIDE_N == G.STRIDE_ROWS + 64 + 1 and G.STRIDE_N > G.REBASE_ROWS and G.STRIDE_N * 9 * 0.9 > G.BYTEMAP_BYTES   # (9-byte rows, a tenth of them null)
