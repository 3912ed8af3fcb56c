// parquet_write.cpp -- one record batch -> one complete Parquet file image in host memory.
//
// Replaces the encode the reference does with the `parquet` crate behind the projection
// (materialize_files_task.rs:128-141: AsyncArrowWriter::try_new(writer, schema, None) / write / close -- one file, one
// row group per record).  Three stages: the DEVICE ENCODE here (plan_row_group: the value streams of the data pages are
// produced in HBM by parquet_write.hip; a non-null fixed-width column needs no kernel, its Arrow buffer IS the PLAIN stream),
// the pure LAYOUT of parquet_layout.cpp (page cuts, page headers, chunk offsets, statistics bytes, the footer), and the
// ASSEMBLY here (assemble_image: every piece copied once into its place in the file image).
// Output format: PLAIN encoding, UNCOMPRESSED, data pages V1 of `parquet_page_rows` rows (default 65 536, at most 64 pages
// per chunk), definition levels = the Arrow validity bitmap behind a one-run header per page, chunk statistics (null_count,
// min_value / max_value, TypeDefinedOrder) like the parquet crate's writer records them.  Any Parquet reader decodes it
// (tests: pyarrow, and this library's own scan); it is NOT byte-identical to what the parquet crate writes (that one
// dictionary-encodes first and adds page indexes).
// Types: Int32, Int64, Float32, Float64, Boolean, Utf8; anything else CHQ_ERR_NOT_SUPPORTED.
#include <cstring>

#include "engine.hpp"
#include "parquet.hpp"
#include "parquet_device.h"

namespace chq {
namespace {
static_assert(PW_LAYOUT_BLOCK_ROWS == PW_BLOCK_ROWS, "the layout cuts pages at the blocks of the stream scan");

// One column of a row group on its way through the encode; the PwChunk of the same index is what the layout is told of it
struct ColumnEncode {
  int stats_kind = 0;                // PwStatsKind
  bool scanned = false;              // the stream is compacted by pw_encode_kernel (Utf8, Boolean, a bitmap that takes part)
  PwParams enc{};                    // enc.validity: the bitmap when it may hold nulls, else null
  const uint8_t* levels = nullptr;   // in HBM: the validity bits from bit 0 (definition levels, bit width 1)
  const uint8_t* stream = nullptr;   // in HBM: the value stream
};
// one row group of the file: the batch on the device, its columns' streams, every device block they lie in
struct RowGroupPlan {
  Batch rec;
  int64_t page_rows = 0;
  std::vector<ColumnEncode> cols;
  std::vector<BufferPtr> keep;
};
struct ReadBack {
  std::vector<unsigned long long> totals;   // per column: bytes of the scanned stream
  std::vector<long long> stats;             // per column: min key / row, max key / row, number of values that took part
};

uint8_t* device_block(Context& ctx, RowGroupPlan& rg, size_t bytes) {
  rg.keep.push_back(make_device_buffer(bytes, ctx.device));
  return (uint8_t*)rg.keep.back()->ptr;
}

// ---- step 1: what kind of column this is (the one type switch) ------------------------------------------------------------
void classify_column(const Column& c, int64_t rows, ColumnEncode& ce, PwChunk& ch) {
  switch (c.type) {
    case T_BOOL: ch.physical = PQ_BOOLEAN; ce.stats_kind = PW_STATS_U8; break;
    case T_I32: ch.physical = PQ_INT32; ce.stats_kind = PW_STATS_I32; break;
    case T_I64: ch.physical = PQ_INT64; ce.stats_kind = PW_STATS_I64; break;
    case T_F32: ch.physical = PQ_FLOAT; ce.stats_kind = PW_STATS_F32; break;
    case T_F64: ch.physical = PQ_DOUBLE; ce.stats_kind = PW_STATS_F64; break;
    case T_UTF8: ch.physical = PQ_BYTE_ARRAY; ce.stats_kind = PW_STATS_UTF8; break;
    default: throw ChqError{CHQ_ERR_NOT_SUPPORTED, "parquet: column '" + c.name + "' of Arrow type '" + c.format + "' (Int32, Int64, Float32, Float64, Boolean and Utf8 are written)"};
  }
  PwParams& e = ce.enc;
  e.n_rows = rows; e.validity = c.live_validity(); e.bit_offset = c.offset;
  if (e.validity && !c.nullable) throw ChqError{CHQ_ERR_ARROW_INVALID_ARGUMENT, "parquet: column '" + c.name + "' is declared non-nullable but carries a validity bitmap"};
  if (c.type == T_UTF8) { e.offsets = (const int32_t*)c.values0(); e.data = c.data; }
  else if (c.type == T_BOOL) e.width = 1;   // (one byte per row first, queue_sizes)
  else { e.width = c.width; e.values = (const uint8_t*)c.values0(); }
  ce.scanned = rows > 0 && (c.type == T_UTF8 || c.type == T_BOOL || e.validity);
  ch.name = c.name; ch.optional = c.nullable; ch.rows = rows;
  ch.has_levels = rows > 0 && e.validity;
}

// ---- step 2: statistics and sizes (scan of the bytes every row contributes), and their way back to the host ------------------
void queue_sizes(Context& ctx, RowGroupPlan& rg, std::vector<PwChunk>& chunks, ReadBack& rb) {
  const int64_t rows = rg.rec.nrows;
  const size_t nc = rg.cols.size();
  const int grid = ctx.num_cus * 8;
  const int64_t n_blocks = std::max<int64_t>(1, (rows + PW_BLOCK_ROWS - 1) / PW_BLOCK_ROWS);
  unsigned long long* totals = (unsigned long long*)device_block(ctx, rg, 8 * (nc + 1));
  check_hip(hipMemsetAsync(totals, 0, 8 * (nc + 1), ctx.stream), "memset");
  // chunk statistics: min / max per column, like the parquet crate's writer (EnabledStatistics default)
  rb.stats.resize(3 * nc);
  for (size_t ci = 0; ci < nc; ++ci) {
    const bool str = rg.cols[ci].stats_kind == PW_STATS_UTF8;
    rb.stats[3 * ci] = str ? -1 : INT64_MAX; rb.stats[3 * ci + 1] = str ? -1 : INT64_MIN; rb.stats[3 * ci + 2] = 0;
  }
  long long* d_stats = (long long*)device_block(ctx, rg, 24 * nc + 16);
  if (nc) check_hip(hipMemcpyAsync(d_stats, rb.stats.data(), 24 * nc, hipMemcpyHostToDevice, ctx.stream), "init statistics");
  for (size_t ci = 0; ci < nc; ++ci) {
    const Column& c = rg.rec.cols[ci];
    ColumnEncode& ce = rg.cols[ci];
    PwParams& e = ce.enc;
    e.n_blocks = n_blocks; e.total_bytes = totals + ci;
    if (c.type == T_BOOL && rows > 0) {   // one byte per row first (any bit offset), compacted in queue_streams like a 1-byte column
      PwParams b{}; b.n_rows = rows; b.values = c.values; b.value_bit_offset = c.offset; b.out = device_block(ctx, rg, (size_t)rows + 64);
      check_hip(pw_launch_bits_to_bytes(b, grid, ctx.stream), "launch pw_bits_to_bytes_kernel");
      e.values = b.out;
    }
    if (rows > 0) {
      PwStatsParams sp{};
      sp.n_rows = rows; sp.validity = e.validity; sp.bit_offset = c.offset; sp.values = e.values;
      sp.offsets = e.offsets; sp.data = e.data; sp.out = d_stats + 3 * ci; sp.kind = ce.stats_kind;
      const int sgrid = (int)std::min<int64_t>((rows + 255) / 256, (int64_t)ctx.num_cus * 4);
      if (c.type == T_UTF8) {
        sp.cand = (long long*)device_block(ctx, rg, (size_t)sgrid * 16 + 16);
        check_hip(pw_launch_stats(sp, sgrid, ctx.stream), "launch pw_stats_kernel");
        sp.n_cand = sgrid;
        check_hip(pw_launch_stats(sp, 1, ctx.stream), "launch pw_stats_kernel (candidates)");
      } else check_hip(pw_launch_stats(sp, sgrid, ctx.stream), "launch pw_stats_kernel");
    }
    if (ce.scanned) {
      e.block_sums = (unsigned long long*)device_block(ctx, rg, (size_t)n_blocks * 8 + 16);
      check_hip(pw_launch_scan(e, ctx.stream), "launch pw_counts_kernel / pw_scan_kernel");
      if (rows > rg.page_rows && c.type != T_BOOL) {   // several pages (a nullable Boolean column stays one): where the blocks start
        chunks[ci].prefix.resize((size_t)n_blocks);
        check_hip(hipMemcpyAsync(chunks[ci].prefix.data(), e.block_sums, (size_t)n_blocks * 8, hipMemcpyDeviceToHost, ctx.stream), "read back block prefix");
      }
    }
  }
  rb.totals.assign(nc + 1, 0);
  check_hip(hipMemcpyAsync(rb.totals.data(), totals, 8 * nc, hipMemcpyDeviceToHost, ctx.stream), "read back");
  if (nc) check_hip(hipMemcpyAsync(rb.stats.data(), d_stats, 24 * nc, hipMemcpyDeviceToHost, ctx.stream), "read back statistics");
}

// ---- step 4: the read-back as a chunk description ------------------------------------------------------------------------------
// The chunk's null count is decided here and nowhere else.  Behind a bitmap the device counted the values (a view's null
// count may be unknown, imported as 1); without one the batch says there are no nulls.
int64_t chunk_null_count(const Column& c, int64_t rows, int64_t values) {
  if (!c.live_validity()) return 0;
  if (rows > 0) return rows - values;
  return c.type == T_UTF8 ? 0 : c.null_count;   // a view without rows: as imported, but a Utf8 chunk has always recorded 0
}

// min_value / max_value of a Utf8 chunk: the bytes of rows `mn` and `mx`
void fetch_string_bounds(const Column& c, long long mn, long long mx, PwChunk& ch) {
  if (mn < 0 || mx < 0) return;
  std::string* dst[2] = {&ch.min_value, &ch.max_value};
  const long long row[2] = {mn, mx};
  for (int k = 0; k < 2; ++k) {
    int32_t o[2];
    check_hip(hipMemcpy(o, (const int32_t*)c.values0() + row[k], 8, hipMemcpyDeviceToHost), "statistics: offsets");
    const int64_t len = (int64_t)o[1] - o[0];
    if (len > 4096) return;   // (a reader gains nothing from a page-sized bound)
    dst[k]->resize((size_t)len);
    if (len) check_hip(hipMemcpy(&(*dst[k])[0], c.data + o[0], (size_t)len, hipMemcpyDeviceToHost), "statistics: bytes");
  }
  ch.has_minmax = true;
}

void describe_chunk(const Column& c, const ColumnEncode& ce, int64_t scanned_bytes, const long long* stats, PwChunk& ch) {
  const int64_t rows = ch.rows;
  const int64_t bytes = rows == 0 ? 0 : ce.scanned ? scanned_bytes : rows * (int64_t)c.width;   // (Boolean: one byte per value)
  if (bytes >= (1ll << 31) - 64) throw ChqError{CHQ_ERR_NOT_SUPPORTED, "parquet: column '" + c.name + "' needs a page of " + std::to_string(bytes) + " bytes"};
  ch.stream_bytes = c.type == T_BOOL ? (bytes + 7) / 8 : bytes;
  const long long mn = stats[0], mx = stats[1], cnt = stats[2];
  ch.null_count = chunk_null_count(c, rows, c.type == T_UTF8 ? cnt : bytes / ce.enc.width);
  if (rows == 0 || cnt == 0) return;   // all null (or all NaN): no min / max
  if (c.type == T_UTF8) fetch_string_bounds(c, mn, mx, ch);
  else parquet_statistics_bytes(mn, mx, ch);
}

// ---- step 5: value streams and level bitmaps in HBM ----------------------------------------------------------------------------
void queue_streams(Context& ctx, RowGroupPlan& rg, const std::vector<PwChunk>& chunks, const ReadBack& rb) {
  const int64_t rows = rg.rec.nrows;
  const int grid = ctx.num_cus * 8;
  for (size_t ci = 0; ci < rg.cols.size(); ++ci) {
    const Column& c = rg.rec.cols[ci];
    ColumnEncode& ce = rg.cols[ci];
    PwParams& e = ce.enc;
    if (!ce.scanned) ce.stream = rows > 0 ? e.values : nullptr;   // the Arrow buffer is the stream
    else {
      const int64_t bytes = (int64_t)rb.totals[ci];
      e.out = device_block(ctx, rg, (size_t)bytes + 64);
      check_hip(pw_launch_encode(e, ctx.stream), "launch pw_encode_kernel");
      ce.stream = e.out;
      if (c.type == T_BOOL) {   // the compacted bytes -> bit-packed
        PwParams b{}; b.n_rows = bytes; b.values = e.out; b.out = device_block(ctx, rg, (size_t)((bytes + 63) / 64) * 8 + 16);
        if (bytes > 0) check_hip(pw_launch_bytes_to_bits(b, grid, ctx.stream), "launch pw_bytes_to_bits_kernel");
        ce.stream = b.out;
      }
    }
    // definition levels (optional columns), bit width 1: the validity bits from bit 0, LSB first (cut per page by the layout)
    if (chunks[ci].has_levels) {
      if ((c.offset & 7) == 0) ce.levels = c.validity + (c.offset >> 3);
      else {
        PwParams b = e; b.out = device_block(ctx, rg, (size_t)((rows + 63) / 64) * 8 + 16);
        check_hip(pw_launch_shift_bits(b, grid, ctx.stream), "launch pw_shift_bits_kernel");
        ce.levels = b.out;
      }
    }
  }
}

// Streams and statistics of ONE batch as one row group: `g` is what the layout needs to know of it
RowGroupPlan plan_row_group(Context& ctx, const Batch& in, PwGroup& g) {
  RowGroupPlan rg;
  rg.rec = to_device(ctx, in);
  const int64_t rows = rg.rec.nrows;
  if (rows >= (1ll << 31)) throw ChqError{CHQ_ERR_NOT_SUPPORTED, "parquet: a batch of " + std::to_string(rows) + " rows in one page"};
  const size_t nc = rg.rec.cols.size();
  g.rows = rows;
  g.chunks.resize(nc);
  rg.cols.resize(nc);
  rg.page_rows = parquet_write_page_rows(ctx.opt_parquet_page_rows, rows);
  for (size_t ci = 0; ci < nc; ++ci) classify_column(rg.rec.cols[ci], rows, rg.cols[ci], g.chunks[ci]);
  ReadBack rb;
  queue_sizes(ctx, rg, g.chunks, rb);
  check_hip(hipStreamSynchronize(ctx.stream), "hipStreamSynchronize");   // step 3: the one wait
  for (size_t ci = 0; ci < nc; ++ci) describe_chunk(rg.rec.cols[ci], rg.cols[ci], (int64_t)rb.totals[ci], &rb.stats[3 * ci], g.chunks[ci]);
  queue_streams(ctx, rg, g.chunks, rb);
  return rg;
}

bool same_schema(const PwGroup& a, const PwGroup& b) {
  bool same = a.chunks.size() == b.chunks.size();
  for (size_t ci = 0; same && ci < a.chunks.size(); ++ci)
    same = a.chunks[ci].name == b.chunks[ci].name && a.chunks[ci].physical == b.chunks[ci].physical && a.chunks[ci].optional == b.chunks[ci].optional;
  return same;
}

// The file image: PAR1, column chunks (pages: header + levels + values) in [4, at), footer, footer length, PAR1.
// The body is assembled in HBM (page heads uploaded as one blob, levels and value streams copied to their file offsets by
// pw_assemble_kernel) and comes down in ONE copy: one copy per page part cost 6 ms for a 4 M-row batch in 62 pages per
// chunk, against 1.6 ms for the single-page form.
ParquetImage assemble_image(Context& ctx, const std::vector<RowGroupPlan>& rgs, const std::vector<PwGroup>& groups, int64_t at, const std::vector<uint8_t>& footer) {
  ParquetImage img;
  img.len = at + (int64_t)footer.size() + 8;
  img.bytes = make_host_buffer((size_t)img.len + 16);
  uint8_t* out = (uint8_t*)img.bytes->ptr;
  memcpy(out, "PAR1", 4);
  if (at > 4) {
    size_t n_pieces = 0, blob_bytes = 0;
    for (const PwGroup& g : groups)
      for (const PwChunkLayout& l : g.layout) for (const PwPage& pg : l.pages) { n_pieces += 1 + (pg.levels_bytes > 0) + (pg.stream_bytes > 0); blob_bytes += pg.head.size(); }
    const size_t pieces_bytes = (n_pieces * sizeof(PwPiece) + 63) & ~(size_t)63;
    std::vector<uint8_t> up(pieces_bytes + blob_bytes);
    auto d_up = make_device_buffer(up.size() + 64, ctx.device);
    auto d_img = make_device_buffer((size_t)at + 64, ctx.device);
    PwPiece* pc = (PwPiece*)up.data();
    size_t k = 0, bo = pieces_bytes;
    unsigned long long longest = 0;
    auto piece = [&](int64_t& p, const uint8_t* src, int64_t bytes) { pc[k++] = PwPiece{(unsigned long long)p, src, (unsigned long long)bytes}; p += bytes; };
    for (size_t gi = 0; gi < groups.size(); ++gi) for (size_t ci = 0; ci < groups[gi].layout.size(); ++ci) {
      const ColumnEncode& ce = rgs[gi].cols[ci];
      int64_t p = groups[gi].layout[ci].at;
      for (const PwPage& pg : groups[gi].layout[ci].pages) {
        memcpy(up.data() + bo, pg.head.data(), pg.head.size());
        piece(p, (const uint8_t*)d_up->ptr + bo, (int64_t)pg.head.size());
        bo += pg.head.size();
        if (pg.levels_bytes) piece(p, ce.levels + pg.levels_at, pg.levels_bytes);
        if (pg.stream_bytes) piece(p, ce.stream + pg.stream_at, pg.stream_bytes);
      }
    }
    for (size_t i = 0; i < n_pieces; ++i) longest = std::max(longest, pc[i].len);
    unsigned long long seg = 256 * 1024;
    while ((longest + seg - 1) / seg > 65535) seg *= 2;
    check_hip(hipMemcpyAsync(d_up->ptr, up.data(), up.size(), hipMemcpyHostToDevice, ctx.stream), "upload page heads");
    PwAssembleParams ap{(const PwPiece*)d_up->ptr, (uint8_t*)d_img->ptr, seg};
    check_hip(pw_launch_assemble(ap, (int)n_pieces, (int)std::max<unsigned long long>(1, (longest + seg - 1) / seg), ctx.stream), "launch pw_assemble_kernel");
    check_hip(hipMemcpyAsync(out + 4, (const uint8_t*)d_img->ptr + 4, (size_t)at - 4, hipMemcpyDeviceToHost, ctx.stream), "copy the file body");
    check_hip(hipStreamSynchronize(ctx.stream), "hipStreamSynchronize");   // (`up` and the device blocks are released by the callers)
  }   // (else: no column, and every row group's plan has waited for what it queued)
  memcpy(out + at, footer.data(), footer.size());
  const uint32_t flen = (uint32_t)footer.size();
  memcpy(out + at + footer.size(), &flen, 4);
  memcpy(out + at + footer.size() + 4, "PAR1", 4);
  return img;
}
}  // namespace

// One file image from one or more batches of the same schema: one row group per batch, in order (the reference writes one
// file per record, materialize_files_task.rs:128-141; several records per file = the row-group compaction its DEV_NOTES.md
// 117-121 asks for).
ParquetImage records_to_parquet(Context& ctx, const std::vector<const Batch*>& ins) {
  if (ins.empty()) throw ChqError{CHQ_ERR_ARROW_INVALID_ARGUMENT, "parquet: no record batch to write"};
  std::vector<RowGroupPlan> rgs;
  std::vector<PwGroup> groups(ins.size());
  for (const Batch* in : ins) {
    if (!in) throw ChqError{CHQ_ERR_INVALID_HANDLE, "null record batch"};
    rgs.push_back(plan_row_group(ctx, *in, groups[rgs.size()]));
    if (!same_schema(groups.front(), groups[rgs.size() - 1])) throw ChqError{CHQ_ERR_ARROW_INVALID_ARGUMENT, "parquet: record batch " + std::to_string(rgs.size() - 1) + " has another schema than the first (names, types and nullability must agree)"};
  }
  int64_t at = 4;
  for (size_t gi = 0; gi < groups.size(); ++gi) parquet_layout_group(groups[gi], rgs[gi].page_rows, at);
  return assemble_image(ctx, rgs, groups, at, parquet_write_footer(groups));
}

ParquetImage record_to_parquet(Context& ctx, const Batch& in) { return records_to_parquet(ctx, std::vector<const Batch*>{&in}); }

}  // namespace chq
