"""The host half of the forged-snappy tests (tests/snappy_forge.py, tests/snappy_forged_cases.py), no GPU: the element
encoder and the strict decoder agree with pyarrow's snappy codec on thousands of seeded scripts and reject the same damage,
the Thrift re-packer reproduces pyarrow's files byte for byte, and every forged file of the GPU tier has the shape its
builder names, reads back in pyarrow as the original table and opens in the library's metadata reader."""
import io

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

import chapterhouseqe_amd as chq
from tests import snappy_forge as F
from tests.snappy_forged_cases import CASES, DAMAGED, build


def random_script(rng: np.random.Generator):
    """a few elements of every spelling: literals with any legal header width, copies through every tag that can hold them
    (lengths 1 to 64, offsets from 1 to the whole output, self-overlapping ones)"""
    elems, out = [], 0
    for _ in range(int(rng.integers(1, 30))):
        if out == 0 or rng.random() < 0.4:
            ln = int(rng.choice([1, 2, 59, 60, 61, 64, 65, 256, 257, 300])) if rng.random() < 0.3 else int(rng.integers(1, 40))
            nb = int(rng.integers(F.min_nb(ln), 5))
            elems.append(F.Lit(rng.bytes(ln), nb if rng.random() < 0.5 else None))
        else:
            off = int(rng.integers(1, out + 1)) if rng.random() < 0.7 else int(rng.integers(1, min(out, 8) + 1))
            ln = int(rng.integers(1, 65))
            kinds = [k for k in (1, 2, 4) if (k != 1 or (4 <= ln <= 11 and off < 2048)) and (k != 2 or off < 65536)]
            elems.append(F.Copy(ln, off, int(rng.choice(kinds))))
        out += elems[-1].length
    return elems


def pa_rejects(stream: bytes, dlen: int) -> bool:
    try:
        F.pa_decompress(stream, dlen)
    except (pa.ArrowException, OSError, ValueError):
        return True
    return False


def test_scripts_round_trip_against_pyarrow():
    rng = np.random.default_rng(12345)
    for _ in range(3000):
        elems = random_script(rng)
        n = F.out_len(elems)
        pre = int(rng.integers(len(F.varint(n)), 6))
        s = F.encode(elems, preamble=pre)
        out, got = F.decode(s, expect=n)
        assert out == F.pa_decompress(s, n)
        # the decoder reports every element where the encoder put it, spelled the same way
        pos, at = pre, 0
        for e, g in zip(elems, got):
            assert (g.in_pos, g.out_pos, g.length) == (pos, at, e.length)
            if isinstance(e, F.Copy):
                assert g.kind == (e.kind or F.min_kind(e.length, e.offset)) and g.offset == e.offset
            else:
                assert g.kind == 0 and g.nb == (F.min_nb(e.length) if e.nb is None else e.nb)
            pos += len(F.encode_element(e))
            at += e.length
        assert len(got) == len(elems) and pos == len(s)
        assert F.script(got, s) == [F.Lit(e.data, g.nb) if isinstance(e, F.Lit) else F.Copy(e.length, e.offset, g.kind)
                                    for e, g in zip(elems, got)]


def test_canonical_and_respelled_streams_decode_alike():
    rng = np.random.default_rng(7)
    for k in range(40):
        data = (rng.integers(0, 1 + k * 7, int(rng.integers(1, 200_000))).astype(np.uint8)).tobytes()
        c = F.canonical(data)
        r = F.respell(c, rng, copy4=0.5, short=0.5, wide=0.5, split_lit=0.5)
        g = 37 if len(r) >= 20 else 0     # (a run of zeros is a handful of elements)
        for s in (F.encode(c), F.encode(r), F.encode(F.grow(r, g))):
            assert F.decode(s)[0] == data == F.pa_decompress(s, len(data))
        assert len(F.encode(F.grow(r, g))) == len(F.encode(r)) + g


DAMAGE = ("offset0", "beyond", "trailing_literal", "trailing_tag", "truncated", "declared_high", "declared_low", "past_length")


@pytest.mark.parametrize("damage", DAMAGE)
def test_damaged_scripts_are_rejected_by_both_decoders(damage):
    rng = np.random.default_rng(DAMAGE.index(damage))
    done = 0
    for _ in range(400):
        elems = random_script(rng)
        n = F.out_len(elems)
        copies = [i for i, e in enumerate(elems) if isinstance(e, F.Copy)]
        if damage in ("offset0", "beyond") and not copies:
            continue
        if damage == "offset0":
            i = int(rng.choice(copies))
            elems[i] = F.Copy(elems[i].length, 0, 2 if rng.random() < 0.5 else 4)
            s = F.encode(elems)
        elif damage == "beyond":
            i = int(rng.choice(copies))
            at = F.out_len(elems[:i])
            elems[i] = F.Copy(elems[i].length, at + int(rng.integers(1, 70_000)), 4)
            s = F.encode(elems)
        elif damage == "trailing_literal":
            s = F.encode(elems) + F.encode_element(F.Lit(b"z"))
        elif damage == "trailing_tag":
            s = F.encode(elems) + bytes([int(rng.integers(0, 256))])
        elif damage == "truncated":
            s = F.encode(elems)
            s = s[:len(s) - int(rng.integers(1, len(F.encode_element(elems[-1])) + 1))]
        elif damage == "declared_high":
            s = F.encode(elems, dlen=n + int(rng.integers(1, 5)))
        elif damage == "declared_low":
            s = F.encode(elems, dlen=n - 1)
        else:
            s = F.encode(elems[:-1] + [F.Lit(rng.bytes(elems[-1].length + 1))], dlen=n)
        with pytest.raises(F.SnappyError):
            F.decode(s, expect=n)
        assert pa_rejects(s, n), damage
        done += 1
    assert done > 200


WRITERS = [dict(), dict(use_dictionary=False), dict(data_page_version="2.0"), dict(data_page_size=2000),
           dict(data_page_version="2.0", use_dictionary=False, data_page_size=5000), dict(row_group_size=3000)]


@pytest.mark.parametrize("kw", WRITERS)
def test_repack_reproduces_pyarrows_files(kw):
    """the Thrift reader / writer round-trips every footer and page header pyarrow writes; repack with no change returns
    the file itself, and a repack with re-spelled streams reads back as the same table"""
    rng = np.random.default_rng(3)
    n = 10_000
    t = pa.table({"i": pa.array(rng.integers(0, 100, n), mask=rng.random(n) < 0.2), "s": pa.array(["s%d" % v for v in rng.integers(0, 50, n)]),
                  "f": pa.array(rng.random(n).astype(np.float32)), "nulls": pa.array([None] * n, type=pa.int32())})
    raw = F.write(t, **kw)
    flen = int.from_bytes(raw[-8:-4], "little")
    assert F.thrift_bytes(F.footer(raw)) == raw[-8 - flen:-8]
    for info, payload in F.pages(raw):
        assert len(payload) == info.header.get(3)
    assert F.repack(raw, lambda info, b: None) == raw
    forged = F.repack(raw, F.respeller(5, pre=5, copy4=0.5, short=0.5, wide=0.5))
    assert forged != raw and pq.read_table(io.BytesIO(forged)).equals(t)
    chq.ParquetFile(forged).describe()


def test_planner_model():
    """the numbers of parquet_scan_plan.cpp the builders aim at"""
    B = F.BLOCK
    assert not F.Plan(10**6, 3 * B - 1).indexed and F.Plan(10**6, 3 * B).indexed and not F.Plan(10**6, 3 * B, 0).indexed
    assert F.Plan(65535, 3 * B).n_seg == 1 and F.Plan(65536, 3 * B).n_seg == 2 and F.Plan(65536, 3 * B, 3).n_seg == 1
    assert F.Plan(F.LARGE - 1, 3 * B).n_seg == 15 and F.Plan(F.LARGE, 3 * B).n_seg == 16 and F.Plan(10**7, 3 * B).n_seg == 16
    assert not F.Plan(F.LARGE - 1, 3 * B).large and F.Plan(F.LARGE, 3 * B).large
    p = F.Plan(7 * 32768 + 1000, 3 * B)
    assert p.bounds() == [p.slen * w // 7 for w in range(1, 7)]


@pytest.mark.parametrize("name", list(CASES) + list(DAMAGED))
def test_forged_files_read_back(name):
    """the builders' own assertions prove each stream's shape; here pyarrow reads the file as the table it wrote (or, for
    damage, refuses it), and the library's metadata reader finds pages that tile every chunk"""
    f = build(name)
    assert f.streams
    if f.damaged:
        with pytest.raises((pa.ArrowException, OSError)):
            pq.read_table(io.BytesIO(f.raw))
    else:
        assert pq.read_table(io.BytesIO(f.raw)).equals(f.table)
    text = chq.ParquetFile(f.raw).describe()
    assert text.count("chunk ") == f.table.num_columns * pq.ParquetFile(io.BytesIO(f.raw)).metadata.num_row_groups
