"""The forged snappy files of tests/test_gpu_snappy_forged.py, built on the host (tests/snappy_forge.py).  Every builder
asserts that its stream has the shape it is named for, so the CPU tier (tests/test_snappy_forge.py) proves the shapes and
that pyarrow reads the files; the GPU tier compares the scan with pyarrow on them.

The kernel paths (csrc/parquet_codec.hip, planned by csrc/parquet_scan_plan.cpp) a page can take, by option snappy_blocks:
  0  one wave inflates the whole page (SNAPPY job)
  1  default: pages of 3 * 64 KiB of output and more are walked (INDEX, or SEG + RESOLVE for 64 KiB and more of input),
     inflated one wave per 64 KiB block (BLOCK) and finished (FINISH: redoes the page if a block gave up)
  2  as 1, but every indexed page is redone by its FINISH job
  3  as 1, but the walk is never cut into segments
"""
from __future__ import annotations

import functools

import numpy as np
import pyarrow as pa

from tests.snappy_forge import (BLOCK, LARGE, LEAD, RING_NEAR, Builder, Copy, Forged, Lit, Plan, Stored, DATA_PAGE_V2,
                                DICTIONARY_PAGE, below_block, block_crossers, canonical, decode, element_at, encode,
                                forge_int64, forge_pages, min_nb, positions, respell, respeller, varint)

MODES = (1, 0, 2, 3)     # snappy_blocks of the contexts every case runs on (1: the default context)


# ---- element shapes --------------------------------------------------------------------------------------------------------
def copy4_near_and_overlapping() -> Forged:
    """copy-4 tags at small offsets, and self-overlapping copy-4 copies (offset < length: a run of period `offset`)"""
    b = Builder(np.random.default_rng(101), copy4=0.5)
    while b.out < 300_000:
        b.one()
        if b.rng.random() < 0.1:
            off = int(b.rng.integers(1, 9))
            b.copy(int(b.rng.integers(off + 1, 65)), off, 4, mark="overlap")
    f = forge_int64(b.end())
    el = b.positions()
    assert sum(e.kind == 4 and e.offset < 2048 for e in el) > 1000
    assert all(el[i].kind == 4 and el[i].offset < el[i].length for i in b.marks["overlap"]) and len(b.marks["overlap"]) > 300
    return f


FAR = (RING_NEAR - 1, RING_NEAR, RING_NEAR + 1, 65535, 65536, 65537, 66000, 70_000, 100_000, 262_144, 500_000, 1 << 20)


def far_offsets() -> Forged:
    """offsets around the end of the LDS ring (65 472 +- 1: the last read from the ring / the first from HBM through
    wave_copy), 65 535 (the largest copy-2), 65 536 and beyond (copy-4 only) up to 1 MiB; alone and several in one batch"""
    b = Builder(np.random.default_rng(102))
    b.to_out((1 << 20) + 1000)
    for rep in range(6):
        for off in FAR:
            for kind in ((2, 4) if off < 65536 else (4,)):
                ln = [1, 3, 4, 17, 64, 33][rep]
                b.copy(ln, off, kind, mark=f"far{off}")
                if rep % 2:
                    b.one()
        b.to_out(b.out + 5000)
    f = forge_int64(b.end())
    el = b.positions()
    for off in FAR:
        assert all(el[i].offset == off for i in b.marks[f"far{off}"]) and len(b.marks[f"far{off}"]) >= 6
    assert Plan(len(f.streams[0][1]), b.out).indexed
    return f


def far_offsets_one_wave() -> Forged:
    """offsets beyond the ring in a page of fewer than three blocks: always inflated by one wave (SNAPPY job)"""
    b = Builder(np.random.default_rng(103), pre=3)
    b.to_out(140_000)
    for off in (RING_NEAR, RING_NEAR + 1, 65535, 65536, 70_000, 100_000, 139_000):
        for ln in (1, 2, 5, 64):
            b.copy(ln, off, 4, mark="far")
        b.to_out(b.out + 3000)
    f = forge_int64(b.end())
    assert b.out < 3 * BLOCK and not Plan(len(f.streams[0][1]), b.out).indexed
    assert sum(e.offset > RING_NEAR for e in b.positions()) >= 20
    return f


def short_copies() -> Forged:
    """copies of length 1, 2 and 3 (copy-2 and copy-4 tags; the compressor never writes them), dense enough that one batch
    of 64 input bytes holds a dozen"""
    b = Builder(np.random.default_rng(104), short=0.8, copy4=0.4)
    b.to_out(260_000)
    f = forge_int64(b.end())
    el = b.positions()
    assert {e.length for e in el if e.kind} >= {1, 2, 3} and sum(e.kind and e.length < 4 for e in el) > 10_000
    assert {e.kind for e in el if e.kind and e.length < 4} == {2, 4}
    return f


LIT_LENGTHS = (1, 60, 61, 64, 65, 4096, 4097, 70_000)


def literal_headers() -> Forged:
    """literals of lengths 1, 60, 61, 64, 65, 4 096, 4 097 and 70 000 with every header the format allows for them: from
    the minimal one up to tag 63 with four length bytes"""
    b = Builder(np.random.default_rng(105))
    b.to_out(300)
    for ln in LIT_LENGTHS:
        for nb in range(min_nb(ln), 5):
            b.lit(b.rng.bytes(ln), nb, mark=f"lit{ln}")
            for _ in range(5):
                b.one()
    b.to_out(b.out + 100_000)
    f = forge_int64(b.end())
    el = b.positions()
    for ln in LIT_LENGTHS:
        got = sorted(el[i].nb for i in b.marks[f"lit{ln}"])
        assert got == list(range(min_nb(ln), 5)) and all(el[i].length == ln for i in b.marks[f"lit{ln}"])
    return f


# ---- block rules -----------------------------------------------------------------------------------------------------------
def literal_across_blocks() -> Forged:
    """literals across output byte k * 65536: a short one inside a batch, one longer than a batch (moved on its own) and one
    of 70 000 bytes that spans a whole block; the INDEX walk reports `aligned = false` and FINISH redoes the page"""
    b = Builder(np.random.default_rng(106))
    for k, ln in ((1, 40), (2, 300), (3, 70_000)):
        b.to_out(k * BLOCK - ln // 2)
        b.lit(b.rng.bytes(ln), mark="cross")
    b.to_out(b.out + 50_000)
    f = forge_int64(b.end())
    el = b.positions()
    assert {el[i] for i in b.marks["cross"]} <= set(block_crossers(el)) and len(b.marks["cross"]) == 3
    return f


def copy_across_blocks() -> Forged:
    """copies across output byte k * 65536 (copy-1, copy-2, copy-4; one of length 2 that ends one byte into the block)"""
    b = Builder(np.random.default_rng(107))
    for k, (ln, off, kind, back) in enumerate([(8, 300, 1, 4), (40, 5000, 2, 20), (64, 30_000, 4, 1), (2, 7, 4, 1)], start=1):
        b.to_out(k * BLOCK - back)
        b.copy(ln, off, kind, mark="cross")
    b.to_out(b.out + 30_000)
    f = forge_int64(b.end())
    el = b.positions()
    assert all(el[i] in block_crossers(el) for i in b.marks["cross"]) and len(b.marks["cross"]) == 4
    return f


def copy_from_previous_block() -> Forged:
    """no element crosses a block boundary, but copies just behind a boundary read bytes of the previous block (the BLOCK
    job meets an offset that reaches below its block, gives up, and FINISH redoes the page)"""
    b = Builder(np.random.default_rng(108))
    for k in (1, 2, 3, 4):
        b.to_out(k * BLOCK)
        b.lit(b.rng.bytes(5))
        b.copy(30, 100 * k, mark="back")
    b.to_out(b.out + 20_000)
    f = forge_int64(b.end())
    el = b.positions()
    assert not block_crossers(el)
    assert all(el[i] in below_block(el) for i in b.marks["back"])
    return f


def _utf8_of_size(n_bytes: int, seed: int) -> pa.Table:
    """a required Utf8 column whose PLAIN page is exactly n_bytes long (4 + length per value)"""
    rng = np.random.default_rng(seed)
    n = n_bytes // 40
    lens = rng.integers(10, 60, n)
    lens[-1] += n_bytes - 4 * n - int(lens.sum())
    assert lens[-1] >= 0
    words = ["alpha", "beta", "gamma", "delta", "x", "yy", "zeta", "the quick brown fox"]
    s = ["".join(words[w] for w in rng.integers(0, len(words), 12))[:k].ljust(int(k), "_") for k in lens]
    return pa.table({"s": pa.array(s)}, schema=pa.schema([pa.field("s", pa.utf8(), nullable=False)]))


def dst_len_around_three_blocks(dlen: int) -> Forged:
    """pages of 3 * 65536 - 1, 3 * 65536 and 3 * 65536 + 1 bytes: the smallest size the scan inflates block by block"""
    t = _utf8_of_size(dlen, dlen)
    f = forge_pages(t, respeller(dlen, copy4=0.3, short=0.3, wide=0.3), use_dictionary=False, data_page_size=1 << 26)
    (info, s), = f.streams
    assert info.uncompressed == dlen and Plan(len(s), dlen).indexed == (dlen >= 3 * BLOCK)
    return f


# ---- segment rules ---------------------------------------------------------------------------------------------------------
def compressed_size(slen: int) -> Forged:
    """a page of exactly `slen` compressed bytes: 65 535 (one INDEX walk), 65 536 (the first size walked in two segments),
    524 287 (16 segments, the last size of an ordinary chain), 524 288 and 524 289 (the wave's "large" chain)"""
    b = Builder(np.random.default_rng(slen), pre=4, copy4=0.2, short=0.05)
    s = b.end(slen)
    f = forge_int64(s)
    p = Plan(slen, b.out)
    assert len(s) == slen and p.indexed and p.large == (slen >= LARGE)
    assert p.n_seg == min(16, slen >> 15) and (p.n_seg >= 2) == (slen >= 65536)
    return f


SEG_SLEN = 7 * 32768 + 1000      # seven segments of 32 KiB and more


def segment_bounds(where: str) -> Forged:
    """every segment bound b_w (w = 1..6) falls exactly on an element start, inside the 5-byte header of a copy-4, or inside
    the 5-byte header of a tag-63 literal"""
    b = Builder(np.random.default_rng({"start": 1, "copy4": 2, "tag63": 3}[where]), pre=4)
    p = Plan(SEG_SLEN, 3 * BLOCK)
    r = {}
    for w, bw in enumerate(p.bounds(), start=1):
        r[w] = 0 if where == "start" else 1 + w % 4
        b.to_in(bw - r[w])
        if where == "tag63":
            b.lit(b.rng.bytes(int(b.rng.integers(1, 300))), 4, mark="at")
        else:
            b.copy(int(b.rng.integers(1, 65)), int(b.rng.integers(1, 5000)), 4 if where == "copy4" else None, mark="at")
    s = b.end(SEG_SLEN)
    f = forge_int64(s)
    p = Plan(SEG_SLEN, b.out)
    assert p.n_seg == 7 and p.indexed
    el = b.positions()
    for w, bw in enumerate(p.bounds(), start=1):
        e = element_at(el, bw)
        assert e.in_pos == bw - r[w] and e == el[b.marks["at"][w - 1]]
        if where == "copy4":
            assert e.kind == 4 and e.hdr == 5
        if where == "tag63":
            assert e.kind == 0 and e.nb == 4 and e.hdr == 5
    return f


def literal_covers_segment() -> Forged:
    """one 70 000-byte literal holds a whole segment and the lead-in of the next: that guess starts inside the literal's
    bytes and cannot meet the chain, so segment 0 walks the page alone"""
    slen = 4 * 32768 + 5000
    b = Builder(np.random.default_rng(110), pre=4)
    p = Plan(slen, 3 * BLOCK)
    b.to_in(p.bound(1) - 10_000)
    b.lit(b.rng.bytes(70_000), mark="big")
    b.to_out(max(b.out + 1000, 3 * BLOCK + 100))
    s = b.end(slen)
    f = forge_int64(s)
    p = Plan(slen, b.out)
    big = b.element("big")
    assert p.n_seg == 4 and p.indexed
    data0, data1 = big.in_pos + big.hdr, big.in_pos + big.hdr + big.length
    assert data0 <= p.bound(1) - LEAD and p.bound(2) <= data1            # segment 1 and segment 2's lead-in: literal bytes
    return f


def lead_in_reads_as_long_literals() -> Forged:
    """the lead-in window [b_w - 2048, b_w) of every segment w >= 1 is literal bytes 0xFC: read as a header that is a
    tag-63 literal of 4 237 049 085 bytes, longer than the page -- every guess fails, is restarted eight times, and segment
    0 walks the page alone"""
    slen = 5 * 32768 + 3000
    b = Builder(np.random.default_rng(111), pre=4)
    p = Plan(slen, 3 * BLOCK)
    for w, bw in enumerate(p.bounds(), start=1):
        b.to_in(bw - LEAD - 3 - 16)
        b.lit(b"\xfc" * (LEAD + 40), mark="fc")
    b.to_out(max(b.out + 1000, 3 * BLOCK + 100))
    s = b.end(slen)
    f = forge_int64(s)
    p = Plan(slen, b.out)
    assert p.n_seg == 5 and p.indexed
    for w, bw in enumerate(p.bounds(), start=1):
        e = b.element("fc", w - 1)
        assert e.kind == 0 and e.in_pos + e.hdr <= bw - LEAD and bw <= e.in_pos + e.hdr + e.length
        assert s[bw - LEAD:bw] == b"\xfc" * LEAD
    return f


# ---- page forms ------------------------------------------------------------------------------------------------------------
def v1_levels_prefix_from_copies(n: int) -> Forged:
    """a V1 page of an optional column: [4-byte length][definition levels][values].  The length prefix's upper bytes are
    written by copies of length 1, so the descriptor patch must read the prefix after the copies ran (`first4`)"""
    rng = np.random.default_rng(n)
    t = pa.table({"o": pa.array(rng.integers(0, 1 << 40, n), mask=rng.random(n) < 0.3)})
    made = []

    def make(info, data):
        head = [Lit(data[:1])]
        for j in range(1, 4):
            d = next((d for d in range(1, j + 1) if data[j] == data[j - d]), None)
            head.append(Copy(1, d, 4 if j % 2 else 2) if d else Lit(data[j:j + 1]))
        s = encode(head + respell(canonical(data[4:]), rng), preamble=5)
        made.append(sum(isinstance(e, Copy) for e in head))
        return s
    f = forge_pages(t, make, use_dictionary=False, data_page_size=1 << 26)
    (info, s), = f.streams
    assert info.type == 0 and made[0] >= 1
    assert any(e.kind and e.out_pos < 4 for e in decode(s)[1])
    assert Plan(len(s), info.uncompressed).indexed == (n >= 60_000)
    return f


def v2_stored_values() -> Forged:
    """V2 pages of a SNAPPY chunk whose values section is stored (is_compressed = false); the dictionary page stays
    compressed (forged)"""
    rng = np.random.default_rng(112)
    n = 60_000
    t = pa.table({"o": pa.array(rng.integers(0, 1000, n), mask=rng.random(n) < 0.2),
                  "s": pa.array(["w%05d" % v for v in rng.integers(0, 3000, n)], mask=rng.random(n) < 0.1)})
    fwd = respeller(113)
    stored = []

    def make(info, data):
        if info.type == DATA_PAGE_V2:
            stored.append(info)
            return Stored(data)
        return fwd(info, data)
    f = forge_pages(t, make, data_page_version="2.0", data_page_size=20_000)
    assert len(stored) >= 4 and all(i.levels for i in stored) and any(i.type == DICTIONARY_PAGE for i, _ in f.streams)
    return f


def v2_empty_values() -> Forged:
    """V2 pages whose values section is empty (an all-null column): the stream is only its preamble, here padded"""
    n = 5000
    t = pa.table({"nulls": pa.array([None] * n, type=pa.int64()), "k": pa.array(np.arange(n) % 13)})
    rng = np.random.default_rng(114)

    def make(info, data):
        if not data:
            return varint(0, 3)
        return encode(respell(canonical(data), rng))
    f = forge_pages(t, make, data_page_version="2.0", use_dictionary=False)
    assert any(s == b"\x80\x80\x00" and i.uncompressed == 0 and i.levels for i, s in f.streams)
    return f


def padded_preambles() -> Forged:
    """every page's uncompressed length written in a padded varint (up to 5 bytes), dictionary pages included"""
    rng = np.random.default_rng(115)
    n = 50_000
    t = pa.table({"a": pa.array(rng.integers(0, 500, n)), "s": pa.array(["v%d" % v for v in rng.integers(0, 999, n)]),
                  "f": pa.array(rng.random(n))})
    f = forge_pages(t, respeller(116, pre=5), data_page_size=30_000)
    assert all(s[:5] == varint(i.uncompressed, 5) for i, s in f.streams) and len(f.streams) > 6
    return f


def dictionary_pages() -> Forged:
    """forged dictionary pages of an Int64 and a Utf8 column (both larger than three blocks: inflated block by block),
    and their data pages, with copy-4, short copies, wide literal headers"""
    rng = np.random.default_rng(117)
    n = 120_000
    t = pa.table({"i": pa.array(rng.integers(0, 40_000, n) * 1_000_003),
                  "s": pa.array(["key-%07d-%s" % (v, "abcdefgh"[v % 8] * (v % 9)) for v in rng.integers(0, 25_000, n)])})
    f = forge_pages(t, respeller(118, copy4=0.4, short=0.3, wide=0.4))
    dicts = [(i, s) for i, s in f.streams if i.type == DICTIONARY_PAGE]
    assert {i.column for i, _ in dicts} == {0, 1}
    assert all(Plan(len(s), i.uncompressed).indexed for i, s in dicts)
    return f


# ---- a seeded random mix ---------------------------------------------------------------------------------------------------
def random_mix(seed: int) -> Forged:
    """Int64 values written by a random script (far offsets, short copies, copy-4, wide headers, elements across blocks),
    a nullable Int32, a Float64 and a Utf8 column re-spelled at random; V1 or V2, dictionaries on or off"""
    rng = np.random.default_rng(1000 + seed)
    b = Builder(rng, max_off=int(rng.choice([60_000, 200_000, 1 << 20])), copy4=float(rng.random()), short=float(rng.random() * 0.4))
    b.to_out(int(rng.integers(20_000, 1_200_000)))
    for _ in range(int(rng.integers(0, 6))):
        b.lit(rng.bytes(int(rng.integers(1, 3000))), int(rng.integers(3, 5)))
        b.to_out(b.out + int(rng.integers(1, 70_000)))
    s = b.end()
    data = decode(s)[0]
    v = np.frombuffer(data, dtype=np.int64)
    n = len(v)
    t = pa.table({
        "a": pa.array(v),
        "b": pa.array(rng.integers(-50, 50, n).astype(np.int32), mask=rng.random(n) < 0.25),
        "c": pa.array(rng.integers(0, 300, n) / 4.0),
        "d": pa.array(["r%d" % x * int(x % 4) for x in rng.integers(0, 20_000, n)]),
    }, schema=pa.schema([pa.field("a", pa.int64(), nullable=False), pa.field("b", pa.int32()), pa.field("c", pa.float64()),
                         pa.field("d", pa.utf8())]))
    other = respeller(2000 + seed, pre=int(rng.integers(3, 6)), copy4=float(rng.random()), short=float(rng.random() * 0.5),
                      wide=float(rng.random()))
    hits = []

    def make(info, page):
        if page == data:
            hits.append(info)
            return s
        return other(info, page)
    kw = dict(data_page_version=str(rng.choice(["1.0", "2.0"])), use_dictionary=["b", "c", "d"] if rng.random() < 0.5 else False,
              data_page_size=int(rng.choice([1 << 26, 1 << 16])) if seed % 3 else 1 << 26)
    f = forge_pages(t, lambda i, p: make(i, p), **kw)
    if kw["data_page_size"] == 1 << 26:
        assert len(hits) == 1
    return f


# ---- damaged streams -------------------------------------------------------------------------------------------------------
DAMAGE = ("offset0", "beyond_block0", "beyond_page", "beyond_small", "past_length", "trailing_literal", "trailing_tag",
          "preamble_high", "preamble_low")


def damaged(kind: str) -> Forged:
    """deliberate damage the scan must report (ChqError), never decode into wrong values: a copy with offset 0; offsets
    beyond the output so far in block 0 of an indexed page (its BLOCK job), in block 2 (a BLOCK job gives up: found by
    FINISH) and in a page of one wave; a last element that runs past the page's uncompressed size; bytes behind the last
    element; a preamble that disagrees with the page header"""
    small = kind == "beyond_small"
    b = Builder(np.random.default_rng(120), pre=4)
    b.to_out(50_000 if small else 2 * BLOCK + 5000)
    at = len(b.elems)
    b.copy(20, 1000)
    b.to_out(b.out + (30_000 if small else 3 * BLOCK))
    good = b.end()
    el = list(b.elems)
    dlen = b.out
    if kind == "offset0":
        el[at] = Copy(20, 0, 2)
    elif kind in ("beyond_page", "beyond_small"):
        el[at] = Copy(20, 2 * BLOCK + 5001 if not small else 50_001, 4)
    elif kind == "beyond_block0":
        el[40] = Copy(8, positions(el, 4)[40].out_pos + 1, 4)
    bad = {"past_length": lambda: encode(el[:-1] + [Lit(el[-1].data + b"\x01")], dlen=dlen, preamble=4),
           "trailing_literal": lambda: good + encode([Lit(b"\x07")])[1:],
           "trailing_tag": lambda: good + b"\xf0",
           "preamble_high": lambda: encode(el, dlen=dlen + 1, preamble=4),
           "preamble_low": lambda: encode(el, dlen=dlen - 1, preamble=4)}.get(kind, lambda: encode(el, preamble=4))()
    assert bad != good
    try:
        decode(bad, expect=dlen)
    except ValueError:
        pass
    else:
        raise AssertionError(f"{kind}: the strict decoder accepts the damage")
    f = forge_int64(bad, damaged_from=good)
    assert Plan(len(bad), dlen).indexed == (not small)
    return f


# ---- the catalogue -----------------------------------------------------------------------------------------------------------
CASES = {
    "copy4_near_and_overlapping": copy4_near_and_overlapping,
    "far_offsets": far_offsets,
    "far_offsets_one_wave": far_offsets_one_wave,
    "short_copies": short_copies,
    "literal_headers": literal_headers,
    "literal_across_blocks": literal_across_blocks,
    "copy_across_blocks": copy_across_blocks,
    "copy_from_previous_block": copy_from_previous_block,
    **{f"dst_len_{d}": functools.partial(dst_len_around_three_blocks, d) for d in (3 * BLOCK - 1, 3 * BLOCK, 3 * BLOCK + 1)},
    **{f"compressed_size_{s}": functools.partial(compressed_size, s) for s in (65535, 65536, LARGE - 1, LARGE, LARGE + 1)},
    **{f"segment_bound_{w}": functools.partial(segment_bounds, w) for w in ("start", "copy4", "tag63")},
    "literal_covers_segment": literal_covers_segment,
    "lead_in_reads_as_long_literals": lead_in_reads_as_long_literals,
    **{f"v1_levels_prefix_from_copies_{n}": functools.partial(v1_levels_prefix_from_copies, n) for n in (5000, 100_000)},
    "v2_stored_values": v2_stored_values,
    "v2_empty_values": v2_empty_values,
    "padded_preambles": padded_preambles,
    "dictionary_pages": dictionary_pages,
    **{f"random_mix_{s}": functools.partial(random_mix, s) for s in range(1, 7)},
}
DAMAGED = {f"damaged_{k}": functools.partial(damaged, k) for k in DAMAGE}


@functools.lru_cache(maxsize=None)
def build(name: str) -> Forged:
    return (CASES.get(name) or DAMAGED[name])()
