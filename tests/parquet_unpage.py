"""An independent page-by-page reader for exactly the files the page encoder (csrc/parquet_write.hip, parquet_write.cpp)
emits: data pages V1, PLAIN, uncompressed, definition levels of bit width 1, flat schema, BOOLEAN / INT32 / INT64 / FLOAT /
DOUBLE / BYTE_ARRAY.  Pure Python + numpy on top of tests/parquet_forge.py (`sections` takes the pages apart, `decode` reads
the level runs); no GPU, no libchq.

  unpage(raw)        every page of every chunk as a Page, after asserting what a reader may rely on (UnpageError otherwise):
                     both sizes of a page header equal the payload, the level length prefix lies inside the payload, as many
                     PLAIN values as set level bits and no byte of the value section left over, every BYTE_ARRAY length prefix
                     ends inside its page, the pages of a chunk tile [data_page_offset, + total_compressed_size), the chunks
                     tile the body from byte 4 to the footer, the pages' num_values sum to the row group's rows
  page_array(page)   the rows of one page as an Arrow array
  reassemble(raw)    one record batch per row group, put together from the pages
tests/test_parquet_unpage.py checks this reader against pyarrow's on files pyarrow wrote."""
from __future__ import annotations

from dataclasses import dataclass
from typing import List

import numpy as np
import pyarrow as pa

from tests import parquet_forge as P
from tests.snappy_forge import DATA_PAGE, TReader, footer

BOOLEAN, INT32, INT64, INT96, FLOAT, DOUBLE, BYTE_ARRAY = range(7)
PLAIN, RLE = 0, 3
FIXED = {INT32: np.dtype("<i4"), INT64: np.dtype("<i8"), FLOAT: np.dtype("<f4"), DOUBLE: np.dtype("<f8")}
ARROW = {BOOLEAN: pa.bool_(), INT32: pa.int32(), INT64: pa.int64(), FLOAT: pa.float32(), DOUBLE: pa.float64(), BYTE_ARRAY: pa.utf8()}


class UnpageError(AssertionError):
    pass


def need(cond, msg: str):
    if not cond:
        raise UnpageError(msg)


@dataclass
class Page:
    row_group: int
    column: int
    page: int                # index inside its chunk
    name: str
    physical: int
    optional: bool
    num_values: int
    levels: np.ndarray       # bool, num_values long (a required column: all True)
    values: object           # fixed widths: numpy view of the page's bytes; BOOLEAN: bool array; BYTE_ARRAY: list of bytes
    header_at: int           # file offsets: page header, payload, first byte behind the page
    payload_at: int
    end: int
    level_bytes: int         # of the level section, its 4-byte length prefix included (required column: 0)
    value_bytes: int


def plain_values(physical: int, data: bytes, count: int, where: str):
    """`count` PLAIN values that fill `data` exactly"""
    if physical in FIXED:
        dt = FIXED[physical]
        need(len(data) == count * dt.itemsize, f"{where}: {count} values of {dt.itemsize} bytes in a value section of {len(data)} bytes")
        return np.frombuffer(data, dtype=dt)
    if physical == BOOLEAN:
        need(len(data) == (count + 7) // 8, f"{where}: {count} Boolean values in a value section of {len(data)} bytes")
        return np.unpackbits(np.frombuffer(data, dtype=np.uint8), bitorder="little")[:count].astype(bool)
    need(physical == BYTE_ARRAY, f"{where}: physical type {physical}")
    out, pos = [], 0
    for k in range(count):
        need(pos + 4 <= len(data), f"{where}: the length prefix of value {k} at {pos} ends behind the page ({len(data)} bytes)")
        ln = int.from_bytes(data[pos:pos + 4], "little")
        need(pos + 4 + ln <= len(data), f"{where}: value {k} at {pos} of {ln} bytes ends behind the page ({len(data)} bytes)")
        out.append(bytes(data[pos + 4:pos + 4 + ln]))
        pos += 4 + ln
    need(pos == len(data), f"{where}: {len(data) - pos} bytes left over behind the last of {count} values")
    return out


def unpage(raw: bytes) -> List[Page]:
    raw = bytes(raw)
    need(len(raw) >= 12 and raw[:4] == b"PAR1" and raw[-4:] == b"PAR1", "no PAR1 at both ends")
    flen = int.from_bytes(raw[-8:-4], "little")
    footer_at = len(raw) - 8 - flen
    need(footer_at >= 4, f"footer of {flen} bytes in a file of {len(raw)}")
    meta = footer(raw)
    schema = meta.get(2)[1]
    need(len(schema) == 1 + schema[0].get(5), "flat schemas only")
    try:
        secs = P.sections(raw)
    except (IndexError, TypeError, ValueError, AssertionError) as e:   # (a chunk that does not start at a page header)
        raise UnpageError(f"the pages cannot be walked: {e!r}") from e
    out: List[Page] = []
    at, k, rows_all = 4, 0, 0
    for gi, rg in enumerate(meta.get(4)[1]):
        rows = rg.get(3)
        rows_all += rows
        cols = rg.get(1)[1]
        need(len(cols) == len(schema) - 1, f"row group {gi}: {len(cols)} chunks for {len(schema) - 1} columns")
        for ci, cc in enumerate(cols):
            md, el = cc.get(3), schema[1 + ci]
            where = f"row group {gi} column {ci}"
            physical, optional, name = md.get(1), el.get(3) == 1, el.get(4).decode()
            need(physical == el.get(1) and physical in ARROW, f"{where}: physical type {physical}, schema {el.get(1)}")
            need(el.get(3) in (0, 1), f"{where}: repetition {el.get(3)}")
            need(md.get(4) == 0, f"{where}: codec {md.get(4)}")
            need(not md.get(11), f"{where}: a dictionary page")
            start, size = md.get(9), md.get(7)
            if size == 0:                          # (pyarrow's chunk of a row group without rows: no page at all)
                need(rows == 0 and md.get(5) == 0 and md.get(6) == 0, f"{where}: an empty chunk for {rows} rows")
                continue
            need(start == at, f"{where}: chunk at {start}, the one before ends at {at}")
            need(md.get(6) == size, f"{where}: total_uncompressed_size {md.get(6)}, total_compressed_size {size}")
            need(md.get(5) == rows, f"{where}: num_values {md.get(5)}, row group of {rows} rows")
            need(start + size <= footer_at, f"{where}: chunk [{start}, {start + size}) runs into the footer at {footer_at}")
            pos, page, total = start, 0, 0
            while pos < start + size:
                w = f"{where} page {page}"
                r = TReader(raw, pos)
                ph = r.struct()
                need(ph.get(1) == DATA_PAGE and ph.get(5) is not None, f"{w}: page type {ph.get(1)}")
                h = ph.get(5)
                nv = h.get(1)
                need(h.get(2) == PLAIN and h.get(3) == RLE, f"{w}: encodings {h.get(2)} / {h.get(3)}")
                need(ph.get(2) == ph.get(3), f"{w}: uncompressed_page_size {ph.get(2)}, compressed_page_size {ph.get(3)}")
                end = r.p + ph.get(3)
                need(end <= start + size, f"{w}: payload [{r.p}, {end}) runs past its chunk's end {start + size}")
                payload = raw[r.p:end]
                need(len(payload) == ph.get(2), f"{w}: payload of {len(payload)} bytes, header says {ph.get(2)}")
                sec = secs[k]
                k += 1
                need((sec.info.row_group, sec.info.column, sec.info.page) == (gi, ci, page) and sec.info.num_values == nv, f"{w}: sections() is at {sec.info}")
                if optional:
                    need(len(payload) >= 4, f"{w}: no room for the level length prefix in {len(payload)} bytes")
                    ll = int.from_bytes(payload[:4], "little")
                    need(4 + ll <= len(payload), f"{w}: level section of {ll} bytes in a payload of {len(payload)}")
                    need(len(sec.levels) == ll and len(sec.values) == len(payload) - 4 - ll, f"{w}: sections() cut {len(sec.levels)} + {len(sec.values)}")
                    try:
                        lv, runs = P.decode(sec.levels, 1, nv)
                    except P.HybridError as e:
                        raise UnpageError(f"{w}: levels: {e}") from e
                    used = runs[-1].pos + runs[-1].hdr + runs[-1].size if runs else 0
                    need(used == ll, f"{w}: the level runs end at {used} of {ll} bytes")
                    levels = lv.astype(bool)
                    level_bytes = 4 + ll
                else:
                    need(sec.levels is None and len(sec.values) == len(payload), f"{w}: sections() found levels in a required column")
                    levels = np.ones(nv, dtype=bool)
                    level_bytes = 0
                values = plain_values(physical, sec.values, int(levels.sum()), w)
                out.append(Page(gi, ci, page, name, physical, optional, nv, levels, values, pos, r.p, end, level_bytes, len(sec.values)))
                total += nv
                pos = end
                page += 1
            need(pos == start + size, f"{where}: the pages end at {pos}, the chunk at {start + size}")
            need(total == rows, f"{where}: the pages hold {total} values, the row group {rows} rows")
            at = start + size
    need(at == footer_at, f"the chunks end at {at}, the footer starts at {footer_at}")
    need(k == len(secs), f"{len(secs) - k} pages more in sections()")
    need(meta.get(3) == rows_all, f"num_rows {meta.get(3)}, the row groups hold {rows_all}")
    return out


def page_array(pg: Page) -> pa.Array:
    """the rows of one page (bit patterns of floats kept; what lies under a null is zero)"""
    n, valid = pg.num_values, pg.levels
    nulls = int(n - valid.sum())
    vbuf = pa.py_buffer(np.packbits(valid, bitorder="little").tobytes()) if pg.optional and nulls else None
    if pg.physical == BYTE_ARRAY:
        lens = np.zeros(n, dtype=np.int64)
        lens[valid] = [len(v) for v in pg.values]
        offs = np.zeros(n + 1, dtype=np.int32)
        np.cumsum(lens, out=offs[1:])
        return pa.StringArray.from_buffers(n, pa.py_buffer(offs.tobytes()), pa.py_buffer(b"".join(pg.values)), vbuf, nulls)
    if pg.physical == BOOLEAN:
        full = np.zeros(n, dtype=bool)
        full[valid] = pg.values
        return pa.Array.from_buffers(pa.bool_(), n, [vbuf, pa.py_buffer(np.packbits(full, bitorder="little").tobytes())], nulls)
    full = np.zeros(n, dtype=FIXED[pg.physical])
    full[valid] = pg.values
    return pa.Array.from_buffers(ARROW[pg.physical], n, [vbuf, pa.py_buffer(full.tobytes())], nulls)


def reassemble(raw: bytes, pages: List[Page] = None) -> List[pa.RecordBatch]:
    pages = unpage(raw) if pages is None else pages
    meta = footer(raw)
    schema = meta.get(2)[1]
    fields = [pa.field(el.get(4).decode(), ARROW[el.get(1)], el.get(3) == 1) for el in schema[1:]]
    out = []
    for gi, _rg in enumerate(meta.get(4)[1]):
        cols = []
        for ci, f in enumerate(fields):
            parts = [page_array(p) for p in pages if (p.row_group, p.column) == (gi, ci)]
            cols.append(pa.concat_arrays(parts) if parts else pa.array([], type=f.type))
        out.append(pa.RecordBatch.from_arrays(cols, schema=pa.schema(fields)))
    return out
