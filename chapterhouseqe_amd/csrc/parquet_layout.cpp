// parquet_layout.cpp -- the Parquet writer's file layout: everything between the device encode and the assembly of
// parquet_write.cpp that is host arithmetic (declarations at the end of parquet.hpp).  Page size, page cuts of the value
// streams and level bitmaps, level runs, Thrift page headers, chunk offsets, statistics bytes, the footer (FileMetaData).
// Standard headers only: tests/parquet_layout_main.cpp builds whole files with it on the CPU, under the host sanitizers.
#include <algorithm>
#include <cstring>

#include "parquet.hpp"

namespace chq {
namespace {

struct ThriftOut {
  std::vector<uint8_t> o;
  std::vector<int> stack;
  int last = 0;
  enum { T_I32 = 5, T_I64 = 6, T_BINARY = 8, T_LIST = 9, T_STRUCT = 12 };
  void byte(uint8_t b) { o.push_back(b); }
  void varint(uint64_t v) { while (v >= 0x80) { byte((uint8_t)(v | 0x80)); v >>= 7; } byte((uint8_t)v); }
  void zigzag(int64_t v) { varint(((uint64_t)v << 1) ^ (uint64_t)(v >> 63)); }
  void field(int id, int type) {
    const int delta = id - last;
    if (delta > 0 && delta <= 15) byte((uint8_t)(delta << 4 | type));
    else { byte((uint8_t)type); zigzag(id); }
    last = id;
  }
  void i32(int id, int64_t v) { field(id, T_I32); zigzag(v); }
  void i64(int id, int64_t v) { field(id, T_I64); zigzag(v); }
  void str(int id, const std::string& s) { field(id, T_BINARY); varint(s.size()); o.insert(o.end(), s.begin(), s.end()); }
  void begin_struct(int id) { field(id, T_STRUCT); stack.push_back(last); last = 0; }
  void begin_element() { stack.push_back(last); last = 0; }   // a struct inside a list: no field header
  void end_struct() { byte(0); last = stack.back(); stack.pop_back(); }
  void list(int id, int elem_type, size_t n) {
    field(id, T_LIST);
    if (n < 15) byte((uint8_t)(n << 4 | elem_type)); else { byte((uint8_t)(0xf0 | elem_type)); varint(n); }
  }
};

int64_t fixed_width(int physical) { return physical == PQ_INT64 || physical == PQ_DOUBLE ? 8 : 4; }

// Rows [r0, r0 + pg.rows) of a chunk cut into pages: the page's slice of the value stream
void cut_stream(const PwChunk& c, int64_t r0, bool last, PwPage& pg) {
  int64_t b0, b1;
  if (c.physical == PQ_BOOLEAN) { b0 = r0 / 8; b1 = (r0 + pg.rows + 7) / 8; }   // (only without a bitmap: every row has a bit)
  else if (c.physical != PQ_BYTE_ARRAY && !c.has_levels) { b0 = r0 * fixed_width(c.physical); b1 = (r0 + pg.rows) * fixed_width(c.physical); }
  else {
    b0 = (int64_t)c.prefix[(size_t)(r0 / PW_LAYOUT_BLOCK_ROWS)];
    b1 = last ? c.stream_bytes : (int64_t)c.prefix[(size_t)((r0 + pg.rows) / PW_LAYOUT_BLOCK_ROWS)];
  }
  pg.stream_at = b0; pg.stream_bytes = b1 - b0;
}

// The level section of an optional column's page, [u32 length][one run]: its host part, and the page's slice of the bitmap
std::vector<uint8_t> level_section(const PwChunk& c, int64_t r0, PwPage& pg) {
  std::vector<uint8_t> run;
  auto varint = [&](uint64_t v) { while (v >= 0x80) { run.push_back((uint8_t)(v | 0x80)); v >>= 7; } run.push_back((uint8_t)v); };
  if (pg.rows == 0) { /* no runs */ }
  else if (c.has_levels) {   // one bit-packed run of ceil(rows / 8) groups
    const int64_t groups = (pg.rows + 7) / 8;
    varint(((uint64_t)groups << 1) | 1u);
    pg.levels_at = r0 / 8; pg.levels_bytes = groups;
  } else { varint((uint64_t)pg.rows << 1); run.push_back(1); }   // one RLE run: `rows` times level 1
  const uint32_t len = (uint32_t)(run.size() + pg.levels_bytes);
  std::vector<uint8_t> lv(4);
  memcpy(lv.data(), &len, 4);
  lv.insert(lv.end(), run.begin(), run.end());
  return lv;
}
}  // namespace

// Several pages per chunk: pages are what a reader decodes in parallel (this library's scan: one workgroup per page), the
// parquet crate cuts them at ~1 MiB.  Page boundaries sit on multiples of 4096 rows (the block size of the stream scan, and a
// whole number of level bytes); at most 64 pages per chunk, so that a file image has a bounded number of pieces.
int64_t parquet_write_page_rows(int64_t opt_page_rows, int64_t rows) {
  const int64_t B = PW_LAYOUT_BLOCK_ROWS;
  int64_t page_rows = std::max<int64_t>(B, opt_page_rows / B * B);
  if (rows > 64 * page_rows) page_rows = ((rows + 63) / 64 + B - 1) / B * B;
  return page_rows;
}

PwChunkLayout parquet_layout_chunk(const PwChunk& c, int64_t page_rows) {
  PwChunkLayout out;
  const int64_t n_pages = std::max<int64_t>(1, (c.rows + page_rows - 1) / page_rows);
  // Boolean values are bit-packed without gaps: behind a null a page would start inside a byte, so such a chunk stays one page
  const bool paged = n_pages > 1 && !(c.physical == PQ_BOOLEAN && c.has_levels);
  const int64_t np = paged ? n_pages : 1;
  for (int64_t k = 0; k < np; ++k) {
    PwPage pg;
    const int64_t r0 = paged ? k * page_rows : 0;
    pg.rows = paged ? std::min(page_rows, c.rows - r0) : c.rows;
    if (c.stream_bytes > 0) {
      if (paged) cut_stream(c, r0, k + 1 == np, pg);
      else pg.stream_bytes = c.stream_bytes;
    }
    std::vector<uint8_t> lv;
    if (c.optional) lv = level_section(c, r0, pg);
    const int64_t payload = (int64_t)lv.size() + pg.levels_bytes + pg.stream_bytes;
    ThriftOut t;
    t.i32(1, PQ_DATA_PAGE); t.i32(2, payload); t.i32(3, payload);
    t.begin_struct(5);
    t.i32(1, pg.rows); t.i32(2, PQ_PLAIN); t.i32(3, PQ_RLE); t.i32(4, PQ_RLE);
    t.end_struct();
    t.byte(0);
    pg.head = std::move(t.o);
    pg.head.insert(pg.head.end(), lv.begin(), lv.end());
    out.bytes += pg.total();
    out.pages.push_back(std::move(pg));
  }
  return out;
}

void parquet_layout_group(PwGroup& g, int64_t page_rows, int64_t& at) {
  g.layout.clear();
  for (const PwChunk& c : g.chunks) {
    g.layout.push_back(parquet_layout_chunk(c, page_rows));
    g.layout.back().at = at;
    at += g.layout.back().bytes;
  }
}

std::vector<uint8_t> parquet_write_footer(const std::vector<PwGroup>& groups) {
  const std::vector<PwChunk>& schema = groups.front().chunks;
  const size_t nc = schema.size();
  int64_t rows_all = 0;
  for (const PwGroup& g : groups) rows_all += g.rows;
  ThriftOut f;
  f.i32(1, 1);
  f.list(2, ThriftOut::T_STRUCT, nc + 1);
  f.begin_element(); f.str(4, "arrow_schema"); f.i32(5, (int64_t)nc); f.end_struct();
  for (const PwChunk& c : schema) {
    f.begin_element();
    f.i32(1, c.physical); f.i32(3, c.optional ? 1 : 0); f.str(4, c.name);
    if (c.physical == PQ_BYTE_ARRAY) { f.i32(6, 0); f.begin_struct(10); f.begin_struct(1); f.end_struct(); f.end_struct(); }   // UTF8 / LogicalType.STRING
    f.end_struct();
  }
  f.i64(3, rows_all);
  f.list(4, ThriftOut::T_STRUCT, groups.size());
  for (const PwGroup& g : groups) {
    f.begin_element();
    f.list(1, ThriftOut::T_STRUCT, nc);
    int64_t total_bytes = 0;
    for (size_t ci = 0; ci < nc; ++ci) {
      const PwChunk& c = g.chunks[ci];
      const PwChunkLayout& l = g.layout[ci];
      f.begin_element();
      f.i64(2, l.at);
      f.begin_struct(3);
      f.i32(1, c.physical);
      f.list(2, ThriftOut::T_I32, 2); f.zigzag(PQ_PLAIN); f.zigzag(PQ_RLE);
      f.list(3, ThriftOut::T_BINARY, 1); f.varint(c.name.size()); f.o.insert(f.o.end(), c.name.begin(), c.name.end());
      f.i32(4, 0); f.i64(5, g.rows); f.i64(6, l.bytes); f.i64(7, l.bytes); f.i64(9, l.at);
      if (c.null_count >= 0 || c.has_minmax) {
        f.begin_struct(12);
        if (c.null_count >= 0) f.i64(3, c.null_count);
        if (c.has_minmax) { f.str(5, c.max_value); f.str(6, c.min_value); }
        f.end_struct();
      }
      f.end_struct();
      f.end_struct();
      total_bytes += l.bytes;
    }
    f.i64(2, total_bytes); f.i64(3, g.rows);
    f.end_struct();
  }
  f.str(6, "chapterhouseqe_amd (MI355X page encoder)");
  // column_orders: TypeDefinedOrder for every column -- without it readers must ignore min_value / max_value
  f.list(7, ThriftOut::T_STRUCT, nc);
  for (size_t ci = 0; ci < nc; ++ci) { f.begin_element(); f.begin_struct(1); f.end_struct(); f.end_struct(); }
  f.byte(0);
  return std::move(f.o);
}

void parquet_statistics_bytes(int64_t min_key, int64_t max_key, PwChunk& c) {
  auto raw = [](const void* v, size_t n) { return std::string((const char*)v, n); };
  // floats travel as the IEEE totalOrder key: the bits, those of a negative number below the sign inverted
  auto unkey32 = [](int64_t k) { int32_t b = (int32_t)k; return (int32_t)(b ^ (int32_t)(((uint32_t)(b >> 31)) >> 1)); };
  auto unkey64 = [](int64_t k) { return (int64_t)(k ^ (int64_t)(((uint64_t)(k >> 63)) >> 1)); };
  switch (c.physical) {
    case PQ_INT32: { int32_t a = (int32_t)min_key, b = (int32_t)max_key; c.min_value = raw(&a, 4); c.max_value = raw(&b, 4); } break;
    case PQ_INT64: c.min_value = raw(&min_key, 8); c.max_value = raw(&max_key, 8); break;
    case PQ_FLOAT: {   // the parquet writers' zero rule: a zero minimum is written as -0.0, a zero maximum as +0.0
      int32_t a = unkey32(min_key), b = unkey32(max_key);
      if ((a & 0x7fffffff) == 0) a = (int32_t)0x80000000;
      if ((b & 0x7fffffff) == 0) b = 0;
      c.min_value = raw(&a, 4); c.max_value = raw(&b, 4); } break;
    case PQ_DOUBLE: {
      int64_t a = unkey64(min_key), b = unkey64(max_key);
      if ((a & 0x7fffffffffffffffLL) == 0) a = (int64_t)0x8000000000000000ULL;
      if ((b & 0x7fffffffffffffffLL) == 0) b = 0;
      c.min_value = raw(&a, 8); c.max_value = raw(&b, 8); } break;
    default: { uint8_t a = (uint8_t)min_key, b = (uint8_t)max_key; c.min_value = raw(&a, 1); c.max_value = raw(&b, 1); } break;   // Boolean
  }
  c.has_minmax = true;
}

}  // namespace chq
