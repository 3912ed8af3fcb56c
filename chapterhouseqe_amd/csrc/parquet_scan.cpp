// parquet_scan.cpp -- orchestration of the GPU page decode (parquet.hip) over the host plans of parquet_scan_plan.cpp: per
// column fetch, plan and upload; per wave the inflate chains and the decode launches.  See parquet.hpp for scope.
#include <algorithm>
#include <cstring>

#include "engine.hpp"
#include "parquet.hpp"
#include "parquet_device.h"

namespace chq {
namespace {

[[noreturn]] void unsupported(const std::string& what) { throw ChqError{CHQ_ERR_NOT_SUPPORTED, "parquet: " + what}; }
[[noreturn]] void malformed(const std::string& what) { throw ChqError{CHQ_ERR_ARROW_INVALID_ARGUMENT, "parquet: " + what}; }

struct Scalars {   // per column, on the device and read back once per phase
  uint32_t err, total_values;
  unsigned long long total_bytes;
};

struct ColumnWork {
  const PqColumnSchema* schema = nullptr;
  PqColumnClass k;
  // The plan is also the source of the column's asynchronous uploads (page table, page lists, dictionary positions): pageable
  // host memory the copy engine may read after the call that queued the copy has returned, so it lives as long as the wave --
  // and so does a chunk fetched through the range reader.
  PqColumnPlan plan;
  BufferPtr fetched;
  std::vector<PqPage> pages;     // the chunk's page headers (parsed here for a file behind a range reader)
  int64_t rows = 0;
  BufferPtr chunkb, pages_dev, nonnull, value_base, valid8, row_val, dense, vsrc, vlen, dict_src, dict_len, offsets, block_sums;
  BufferPtr rawb;                // a compressed chunk as it lies in the file (chunkb is then its uncompressed image)
  BufferPtr plain_dev, dict_dev, rle_dev;   // the page lists
  int64_t uploaded = 0;          // file bytes sent to the GPU for this column
};

struct RowGroupJob {   // one row group between its two phases
  int64_t rows = 0;
  std::vector<ColumnWork> work;
  BufferPtr scal;                 // Scalars per column, on the device
  std::vector<Scalars> hs;        // ... and read back
};

// Everything a wave has queued work against.  The streams may still be reading any of it when an error unwinds the call (a
// malformed second row group, a HIP error): the destructor waits for every stream FIRST and only then lets the members go,
// whatever order they were filled in.
struct Wave {
  Context& ctx;
  std::vector<RowGroupJob> jobs;
  std::vector<PqCodecJob> inflate;   // the inflate jobs of every compressed page, in the order their columns were planned
  struct Col { size_t j, ci; hipEvent_t uploaded, inflated; };   // a column with decode kernels to queue
  std::vector<Col> cols;
  std::vector<std::vector<PqCodecJob>> job_lists;   // as uploaded: sources of asynchronous copies
  std::vector<BufferPtr> device_keep;               // index tables and job lists of the inflate launches
  size_t n_events = 0;                              // of ctx.upload_events in use

  Wave(Context& c, size_t n) : ctx(c), jobs(n) {}
  Wave(const Wave&) = delete;
  ~Wave() {
    for (int i = 0; i < Context::kAuxStreams; ++i) if (ctx.aux[i]) (void)hipStreamSynchronize(ctx.aux[i]);
    (void)hipStreamSynchronize(ctx.stream);
  }
  hipEvent_t next_event() {   // (created on first use, kept with the context)
    const size_t k = n_events++;
    while (ctx.upload_events.size() <= k) {
      hipEvent_t e = nullptr;
      check_hip(hipEventCreateWithFlags(&e, hipEventDisableTiming), "hipEventCreate");
      ctx.upload_events.push_back(e);
    }
    return ctx.upload_events[k];
  }
};

// (`v` is read when the copy runs: a member of the wave)
template <typename T>
BufferPtr upload(Context& ctx, hipStream_t stream, const std::vector<T>& v) {
  auto b = make_device_buffer(v.size() * sizeof(T) + 16, ctx.device);
  if (!v.empty()) check_hip(hipMemcpyAsync(b->ptr, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, stream), "upload page table");
  return b;
}

// The stream of column `ci` of the `j`-th row group of a wave.  (ci + j * columns) % 12 put the same column of consecutive
// row groups on 12 / gcd(columns, 12) ... streams -- three columns: the string column of twenty row groups shared FOUR streams,
// and its pages (the slow ones: serial walks, serial inflates) queued five deep.  7 and 5 are coprime with 12: the columns of one
// row group get distinct streams, and one column visits all twelve over twelve row groups.
inline hipStream_t column_stream(Context& ctx, size_t ci, size_t j) { return ctx.aux[(ci * 7 + j * 5) % Context::kKernelStreams]; }

// ---- phase A: everything up to the Utf8 offsets, the columns side by side on the auxiliary streams (already forked) -----
// One column: its chunk's bytes (where they lie in the caller's memory, or fetched through the caller's range reader --
// exactly this chunk: columns a call does not ask for are never read), the plan, every upload on the copy stream, one event.
void queue_column(Context& ctx, const PqFile& f, const PqColumnChunk& cc, Wave& wave, size_t j, size_t ci) {
  const hipStream_t ustream = ctx.aux[Context::kCopyStream];   // every upload of the call (see engine.hpp)
  ColumnWork& w = wave.jobs[j].work[ci];
  const PqColumnSchema& cs = *w.schema;
  const int64_t rows = w.rows;
  w.k = parquet_classify_column(cs, cc, rows, f.size);
  const int64_t first = w.k.first, csize = w.k.csize;
  const uint8_t* chunk_host = nullptr;
  if (csize > 0) {
    if (f.data) chunk_host = f.data + first;
    else {
      w.fetched = make_host_buffer((size_t)csize + 16);
      if (f.read(f.read_user, first, csize, (uint8_t*)w.fetched->ptr) != 0) malformed("the range reader failed on column '" + cs.name + "' (" + std::to_string(csize) + " bytes at " + std::to_string(first) + ")");
      chunk_host = (const uint8_t*)w.fetched->ptr;
    }
  }
  const std::vector<PqPage>* chunk_pages = &cc.pages;
  if (!cc.pages_parsed) {   // (file behind a range reader: the headers are parsed from the bytes just fetched)
    PqColumnChunk tmp = cc;
    if (csize > 0) parquet_parse_pages(chunk_host, csize, tmp);
    w.pages = std::move(tmp.pages);
    chunk_pages = &w.pages;
  }
  BufferPtr raw = make_device_buffer((size_t)csize + 64, ctx.device);
  if (csize > 0) check_hip(hipMemcpyAsync(raw->ptr, chunk_host, (size_t)csize, hipMemcpyHostToDevice, ustream), "upload column chunk");
  check_hip(hipMemsetAsync((uint8_t*)raw->ptr + csize, 0, 64, ustream), "memset");
  w.uploaded = csize;
  if (!w.k.compressed) w.chunkb = raw; else w.rawb = raw;   // (compressed: chunkb = the uncompressed image, allocated below)

  // (the host's walk over the pages and a dictionary runs while the copy engine moves the chunk)
  w.plan = parquet_plan_column(w.k, cs, *chunk_pages, rows, chunk_host);
  const PqColumnPlan& pl = w.plan;
  const size_t n_pages = pl.descs.size();
  w.pages_dev = upload(ctx, ustream, pl.descs);
  w.nonnull = w.k.has_levels ? make_device_buffer(n_pages * 4 + 16, ctx.device) : upload(ctx, ustream, pl.h_nonnull);
  w.value_base = w.k.has_levels ? make_device_buffer(n_pages * 4 + 16, ctx.device) : upload(ctx, ustream, pl.h_base);
  // (every upload of the column is queued before its first kernel: the column's stream then waits ONCE, on one event)
  w.plain_dev = upload(ctx, ustream, pl.plain_list); w.dict_dev = upload(ctx, ustream, pl.dict_list); w.rle_dev = upload(ctx, ustream, pl.rle_list);
  if (pl.dict_walked) {
    w.dict_src = upload(ctx, ustream, pl.h_src);
    w.dict_len = upload(ctx, ustream, pl.h_len);
  }
  const hipEvent_t ev_uploaded = wave.next_event();
  check_hip(hipEventRecord(ev_uploaded, ustream), "hipEventRecord(upload)");
  if (w.k.compressed) {   // every page is inflated into the image by the inflate launches of the wave's parts (queue_wave)
    w.chunkb = make_device_buffer((size_t)pl.image_bytes + 64, ctx.device);
    check_hip(hipMemsetAsync((uint8_t*)w.chunkb->ptr + pl.image_bytes, 0, 64, ustream), "memset");
    Scalars* dscal = (Scalars*)wave.jobs[j].scal->ptr;
    for (PqCodecJob job : pl.jobs) {
      job.raw = (const uint8_t*)w.rawb->ptr; job.image = (uint8_t*)w.chunkb->ptr; job.pages = (PqPageDesc*)w.pages_dev->ptr; job.err = &dscal[ci].err;
      wave.inflate.push_back(job);
    }
  }
  if (rows == 0 || n_pages == 0) return;   // (an empty row group: phase B builds empty columns)
  wave.cols.push_back(Wave::Col{j, ci, ev_uploaded, nullptr});
}

void queue_row_group(Context& ctx, const PqFile& f, int row_group, Wave& wave, size_t j, const std::vector<int>& sel) {
  if (row_group < 0 || row_group >= (int)f.row_groups.size()) malformed("row group " + std::to_string(row_group) + " of " + std::to_string(f.row_groups.size()));
  const PqRowGroup& rg = f.row_groups[row_group];
  const int64_t rows = rg.num_rows;
  if (rows < 0 || rows >= (1ll << 31)) unsupported("row group of " + std::to_string(rows) + " rows");
  const size_t nc = sel.size();   // the columns this call decodes (work item ci <-> file column sel[ci])
  RowGroupJob& job = wave.jobs[j];
  job.rows = rows;
  job.work.assign(nc, ColumnWork{});
  job.hs.assign(nc + 1, Scalars{});
  for (size_t ci = 0; ci < nc; ++ci) {
    job.work[ci].schema = &f.columns[(size_t)sel[ci]]; job.work[ci].rows = rows;
    queue_column(ctx, f, rg.columns[(size_t)sel[ci]], wave, j, ci);
  }
}

// The column's decode kernels, queued once the wave's uploads and inflate launches are in place.  Nothing but a HIP error
// throws from here on: what a plan can refuse, parquet_plan_column has refused.
void launch_decode(Context& ctx, ColumnWork& w, const PqColumnPlan& pl, hipStream_t cstream, Scalars* dscal) {
  const int64_t rows = w.rows;
  PqDecodeParams p{};
  p.chunk = (const uint8_t*)w.chunkb->ptr; p.pages = (const PqPageDesc*)w.pages_dev->ptr; p.n_pages = (int)pl.descs.size(); p.width = w.k.width;
  p.nonnull = (uint32_t*)w.nonnull->ptr; p.value_base = (uint32_t*)w.value_base->ptr;
  p.total_values = &dscal->total_values; p.err = &dscal->err;
  p.dict_at = pl.dict_at; p.dict_len = pl.dict_len; p.dict_count = pl.dict_count;
  if (w.k.has_levels) {
    w.valid8 = make_device_buffer((size_t)rows + 64, ctx.device);
    w.row_val = make_device_buffer((size_t)rows * 4 + 64, ctx.device);
    p.valid8 = (uint8_t*)w.valid8->ptr; p.row_val = (int32_t*)w.row_val->ptr;
    check_hip(pq_launch_levels(p, cstream), "launch pq_levels_kernel");
    check_hip(pq_launch_page_scan(p, cstream), "launch pq_page_scan_kernel");
    check_hip(pq_launch_rowval(p, cstream), "launch pq_rowval_kernel");
  }
  // dense values: at most `rows` of them
  if (w.k.byte_array) {
    w.vsrc = make_device_buffer((size_t)rows * 4 + 64, ctx.device);
    w.vlen = make_device_buffer((size_t)rows * 4 + 64, ctx.device);
    p.vsrc = (uint32_t*)w.vsrc->ptr; p.vlen = (uint32_t*)w.vlen->ptr;
    if (!pl.dict_list.empty()) {
      if (w.k.compressed) {   // the page is only readable after inflation: one workgroup walks it on the device
        w.dict_src = make_device_buffer((size_t)pl.dict_count * 4 + 16, ctx.device);
        w.dict_len = make_device_buffer((size_t)pl.dict_count * 4 + 16, ctx.device);
        PqDecodeParams dpw = p;
        dpw.walk_dictionary = 1; dpw.dict_src = (uint32_t*)w.dict_src->ptr; dpw.dict_len_out = (uint32_t*)w.dict_len->ptr;
        if (pl.dict_count > 0) check_hip(pq_launch_ba_walk(dpw, 1, cstream), "launch pq_ba_walk_kernel (dictionary)");
      }
      p.dict_src = (uint32_t*)w.dict_src->ptr; p.dict_len_out = (uint32_t*)w.dict_len->ptr;
      p.page_list = (const int32_t*)w.dict_dev->ptr;
      check_hip(pq_launch_dict_ba(p, (int)pl.dict_list.size(), cstream), "launch pq_dict_ba_kernel");
    }
    if (!pl.plain_list.empty()) {
      p.page_list = (const int32_t*)w.plain_dev->ptr;
      check_hip(pq_launch_ba_walk(p, (int)pl.plain_list.size(), cstream), "launch pq_ba_walk_kernel");
    }
    // offsets = exclusive scan of the row lengths
    w.offsets = make_device_buffer((size_t)(rows + 2) * 4, ctx.device);
    const int64_t n_blocks = (rows + PQ_SCAN_ROWS - 1) / PQ_SCAN_ROWS;
    w.block_sums = make_device_buffer((size_t)n_blocks * 8 + 16, ctx.device);
    PqRowParams r{};
    r.n_rows = rows; r.row_val = w.k.has_levels ? (const int32_t*)w.row_val->ptr : nullptr;
    r.vlen = (const uint32_t*)w.vlen->ptr; r.out = w.offsets->ptr;
    r.block_sums = (unsigned long long*)w.block_sums->ptr; r.n_blocks = n_blocks; r.total_bytes = &dscal->total_bytes;
    check_hip(pq_launch_rowlen(r, cstream), "launch pq_rowlen kernels");
  } else {
    w.dense = make_device_buffer((size_t)rows * w.k.width + 64, ctx.device);
    p.dense = (uint8_t*)w.dense->ptr;
    if (!pl.plain_list.empty()) {
      p.page_list = (const int32_t*)w.plain_dev->ptr;
      if (w.k.boolean) check_hip(pq_launch_bool(p, (int)pl.plain_list.size(), cstream), "launch pq_bool_kernel");
      else check_hip(pq_launch_plain_copy(p, (int)pl.plain_list.size(), cstream), "launch pq_plain_copy_kernel");
    }
    if (!pl.rle_list.empty()) {
      p.page_list = (const int32_t*)w.rle_dev->ptr;
      check_hip(pq_launch_bool_rle(p, (int)pl.rle_list.size(), cstream), "launch pq_bool_rle_kernel");
    }
    if (!pl.dict_list.empty()) {
      p.page_list = (const int32_t*)w.dict_dev->ptr;
      check_hip(pq_launch_dict_fixed(p, (int)pl.dict_list.size(), cstream), "launch pq_dict_fixed_kernel");
    }
  }
}

// One chain of inflate launches on `st`, behind everything uploaded so far; the event behind its last launch.
hipEvent_t launch_chain(Context& ctx, Wave& wave, const PqChain& ch, hipStream_t st) {
  const hipStream_t ustream = ctx.aux[Context::kCopyStream];
  wave.job_lists.push_back(ch.flat());
  std::vector<PqCodecJob>& list = wave.job_lists.back();
  if (ch.words) {   // (the jobs carry offsets into the table until it exists)
    BufferPtr index_dev = make_device_buffer(ch.words * sizeof(uint32_t) + 16, ctx.device);
    check_hip(hipMemsetAsync(index_dev->ptr, 0, ch.words * sizeof(uint32_t), ustream), "memset");
    for (PqCodecJob& j : list) if (j.codec >= PQ_CODEC_SNAPPY_INDEX) j.index = (uint32_t*)((uint8_t*)index_dev->ptr + (uintptr_t)j.index);
    wave.device_keep.push_back(index_dev);
  }
  BufferPtr jobs_dev = make_device_buffer(list.size() * sizeof(PqCodecJob) + 16, ctx.device);
  check_hip(hipMemcpyAsync(jobs_dev->ptr, list.data(), list.size() * sizeof(PqCodecJob), hipMemcpyHostToDevice, ustream), "upload inflate jobs");
  wave.device_keep.push_back(jobs_dev);
  // the chain starts behind everything uploaded so far: the pages, the job list, the cleared index table
  const hipEvent_t ev_ready = wave.next_event();
  check_hip(hipEventRecord(ev_ready, ustream), "hipEventRecord(jobs)");
  check_hip(hipStreamWaitEvent(st, ev_ready, 0), "hipStreamWaitEvent(jobs)");
  const PqCodecJob* at = (const PqCodecJob*)jobs_dev->ptr;
  const size_t counts[4] = {ch.seg.size(), ch.index.size(), ch.blocks.size(), ch.finish.size()};
  for (int k = 0; k < 4; ++k) {
    PqCodecParams cp{};
    cp.jobs = at; cp.n_jobs = (int32_t)counts[k];
    check_hip(k < 2 ? pq_launch_inflate_index(cp, st) : pq_launch_inflate(cp, st), "launch pq_inflate_kernel");
    at += counts[k];
  }
  const hipEvent_t ev_done = wave.next_event();
  check_hip(hipEventRecord(ev_done, st), "hipEventRecord(inflate)");
  return ev_done;
}

// Phase A of a wave.  The compressed pages are inflated in up to three PARTS of consecutive row groups, each behind the
// uploads of its own row groups (the GPU would otherwise idle until the wave's last upload); the decode kernels of a part's
// columns wait for that part's event.
//   A snappy page of several 64 KiB blocks is inflated block by block (parquet_codec.hip): an INDEX job walks its element
// chain and notes where each block starts, one BLOCK job per block moves the bytes, a FINISH job patches the page
// descriptor (and redoes the page with one wave in the case the format allows and no compressor produces: blocks that
// depend on each other): a CHAIN of three launches in stream order.
//   The INDEX walk is serial per page and its time grows with the page's compressed size, so a few large pages (a 1 MiB
// dictionary page of short strings: 13 ms) would hold back the BLOCK launch of all the others: pages of 512 KiB and more
// of compressed bytes are collected over the whole wave and form ONE more chain on a stream of its own, behind the last
// upload.  (Their walks all have to run side by side -- in one launch: a chain per part put them behind each other on
// the few hardware queues the streams share, 33 -> 51 ms for the 20-row-group sample.)
void queue_wave(Context& ctx, const PqFile& f, int first, Wave& wave, const std::vector<int>& sel) {
  PqChain large;
  const size_t n = wave.jobs.size(), n_parts = parquet_inflate_parts(n);
  size_t job0 = 0, col0 = 0, part = 0;
  for (size_t j = 0; j < n; ++j) {
    queue_row_group(ctx, f, first + (int)j, wave, j, sel);
    if (!parquet_part_ends(j, n_parts, n, part)) continue;
    PqChain ch;
    parquet_route_jobs(wave.inflate.data() + job0, wave.inflate.size() - job0, ctx.opt_snappy_blocks, ch, large);
    hipEvent_t ev = nullptr;
    if (!ch.blocks.empty()) ev = launch_chain(ctx, wave, ch, ctx.aux[(part % 2) * 2]);   // (two streams: a part's INDEX launch next to the BLOCK launch before it)
    for (; col0 < wave.cols.size(); ++col0) wave.cols[col0].inflated = ev;
    job0 = wave.inflate.size(); ++part;
  }
  const hipEvent_t ev_large = large.index.empty() ? nullptr : launch_chain(ctx, wave, large, ctx.aux[1]);
  for (const Wave::Col& c : wave.cols) {
    ColumnWork& w = wave.jobs[c.j].work[c.ci];
    const hipStream_t cstream = column_stream(ctx, c.ci, c.j);
    check_hip(hipStreamWaitEvent(cstream, w.k.compressed && c.inflated ? c.inflated : c.uploaded, 0), "hipStreamWaitEvent(upload)");
    if (w.k.compressed && ev_large) check_hip(hipStreamWaitEvent(cstream, ev_large, 0), "hipStreamWaitEvent(inflate)");
    launch_decode(ctx, w, w.plan, cstream, (Scalars*)wave.jobs[c.j].scal->ptr + c.ci);
  }
}

// ---- phase B: per-row outputs (sizes are on the host now) -----------------------------------------------------------------
Batch phase_b(Context& ctx, RowGroupJob& job, size_t stream_shift) {
  const int64_t rows = job.rows;
  const size_t nc = job.work.size();
  std::vector<ColumnWork>& work = job.work;
  const std::vector<Scalars>& hs = job.hs;
  Batch out;
  out.on_device = true; out.device_id = ctx.device; out.nrows = rows;
  const int grid = ctx.num_cus * 8;
  for (size_t ci = 0; ci < nc; ++ci) {
    const hipStream_t cstream = column_stream(ctx, ci, stream_shift);
    ColumnWork& w = work[ci];
    if (hs[ci].err) malformed(std::string(hs[ci].err == PQ_ERR_CODEC ? "compressed pages" : hs[ci].err == PQ_ERR_LEVELS ? "definition levels" : "values") + " of column '" + w.schema->name + "' are malformed");
    Column o;
    o.name = w.schema->name; o.format = w.k.format; o.nullable = w.schema->repetition == 1; o.length = rows; o.offset = 0;
    parse_arrow_format(w.k.format, &o.type, &o.width);
    const int64_t nonnull = w.k.has_levels && rows > 0 ? (int64_t)hs[ci].total_values : rows;
    o.null_count = rows - nonnull;
    const int32_t* row_val = (w.k.has_levels && o.null_count > 0) ? (const int32_t*)w.row_val->ptr : nullptr;
    if (rows == 0) {
      auto vb = make_device_buffer(64, ctx.device);
      check_hip(hipMemsetAsync(vb->ptr, 0, 64, cstream), "memset");
      o.values = (const uint8_t*)vb->ptr; o.owned.push_back(vb);
      if (w.k.byte_array) { auto db = make_device_buffer(64, ctx.device); o.data = (const uint8_t*)db->ptr; o.owned.push_back(db); o.data_bytes = 0; }
      out.cols.push_back(std::move(o));
      continue;
    }
    if (o.null_count > 0) {   // validity bitmap from the one-byte-per-row levels
      auto vb = make_device_buffer((size_t)((rows + 63) / 64) * 8 + 16, ctx.device);
      PqRowParams r{};
      r.n_rows = rows; r.dense = (const uint8_t*)w.valid8->ptr; r.out = vb->ptr;
      check_hip(pq_launch_pack_bits(r, grid, cstream), "launch pq_pack_bits_kernel");
      o.validity = (const uint8_t*)vb->ptr; o.owned.push_back(vb);
    }
    if (w.k.byte_array) {
      const unsigned long long total = hs[ci].total_bytes;
      if (total >= (1ull << 31)) throw ChqError{CHQ_ERR_ARROW_INVALID_ARGUMENT, "offset overflow: column '" + o.name + "' of this row group holds " + std::to_string(total) + " bytes; Utf8 offsets are int32"};
      auto db = make_device_buffer((size_t)total + 64, ctx.device);
      PqRowParams r{};
      r.n_rows = rows; r.row_val = row_val; r.vsrc = (const uint32_t*)w.vsrc->ptr; r.vlen = (const uint32_t*)w.vlen->ptr;
      r.chunk = (const uint8_t*)w.chunkb->ptr; r.offsets = w.offsets->ptr; r.data_out = (uint8_t*)db->ptr;
      check_hip(pq_launch_utf8_copy(r, grid, cstream), "launch pq_utf8_copy_kernel");
      o.values = (const uint8_t*)w.offsets->ptr; o.owned.push_back(w.offsets);
      o.data = (const uint8_t*)db->ptr; o.owned.push_back(db); o.data_bytes = (int64_t)total;
    } else if (w.k.boolean) {
      auto vb = make_device_buffer((size_t)((rows + 63) / 64) * 8 + 16, ctx.device);
      PqRowParams r{};
      r.n_rows = rows; r.row_val = row_val; r.dense = (const uint8_t*)w.dense->ptr; r.out = vb->ptr;
      check_hip(pq_launch_pack_bits(r, grid, cstream), "launch pq_pack_bits_kernel");
      o.values = (const uint8_t*)vb->ptr; o.owned.push_back(vb);
    } else if (row_val) {
      auto vb = make_device_buffer((size_t)rows * w.k.width + 64, ctx.device);
      PqRowParams r{};
      r.n_rows = rows; r.row_val = row_val; r.dense = (const uint8_t*)w.dense->ptr; r.out = vb->ptr;
      check_hip(pq_launch_gather_fixed(r, w.k.width, grid, cstream), "launch pq_gather_fixed_kernel");
      o.values = (const uint8_t*)vb->ptr; o.owned.push_back(vb);
    } else {   // no nulls: the dense values ARE the column
      o.values = (const uint8_t*)w.dense->ptr; o.owned.push_back(w.dense);
    }
    out.cols.push_back(std::move(o));
  }
  return out;
}

// One wave: both phases, a host synchronisation behind each.  The streams are forked off ctx.stream and joined back into it
// with events (memory.cpp: fork_aux_streams / join_aux_streams).
void run_wave(Context& ctx, const PqFile& f, int first, int end, const std::vector<int>& sel, std::vector<Batch>& outs) {
  Wave wave(ctx, (size_t)(end - first));
  for (RowGroupJob& job : wave.jobs) {
    job.scal = make_device_buffer(sizeof(Scalars) * (sel.size() + 1), ctx.device);
    check_hip(hipMemsetAsync(job.scal->ptr, 0, sizeof(Scalars) * (sel.size() + 1), ctx.stream), "memset");
  }
  fork_aux_streams(ctx);
  queue_wave(ctx, f, first, wave, sel);
  join_aux_streams(ctx);
  for (RowGroupJob& job : wave.jobs)
    if (!job.work.empty()) check_hip(hipMemcpyAsync(job.hs.data(), job.scal->ptr, sizeof(Scalars) * job.work.size(), hipMemcpyDeviceToHost, ctx.stream), "read back");
  check_hip(hipStreamSynchronize(ctx.stream), "hipStreamSynchronize");
  fork_aux_streams(ctx);
  for (size_t j = 0; j < wave.jobs.size(); ++j) {
    outs.push_back(phase_b(ctx, wave.jobs[j], j));
    // (chq_call_stats of a scan: rows decoded, file bytes sent to the GPU, Arrow bytes produced)
    ctx.stats.rows_in += wave.jobs[j].rows; ctx.stats.rows_out += wave.jobs[j].rows;
    for (const ColumnWork& w : wave.jobs[j].work) ctx.stats.bytes_read_alg += w.uploaded;
  }
  join_aux_streams(ctx);
  check_hip(hipStreamSynchronize(ctx.stream), "hipStreamSynchronize");   // the temporaries of the wave are released here
}

}  // namespace

// Row groups [first, first + count): phase A of all of them is in flight before the first size is read back, so the two
// host synchronisations are paid once per call (per wave of about 1 GiB of column chunks), not once per row group, and the
// upload of one row group overlaps the decode of the previous ones.  Only the columns in `columns` are fetched and decoded.
std::vector<Batch> parquet_read_row_groups(Context& ctx, const PqFile& f, int first, int count, const int32_t* columns, int n_columns) {
  if (first < 0 || count < 0 || first + count > (int)f.row_groups.size())
    malformed("row groups [" + std::to_string(first) + ", " + std::to_string(first + count) + ") of " + std::to_string(f.row_groups.size()));
  std::vector<int> sel;
  if (!columns || n_columns < 0) { for (size_t i = 0; i < f.columns.size(); ++i) sel.push_back((int)i); }
  else {
    for (int k = 0; k < n_columns; ++k) {
      if (columns[k] < 0 || columns[k] >= (int)f.columns.size())
        throw ChqError{CHQ_ERR_ARROW_INVALID_ARGUMENT, "parquet: column index " + std::to_string(columns[k]) + " of " + std::to_string(f.columns.size())};
      sel.push_back(columns[k]);
    }
  }
  ctx.stats = chq_call_stats{};
  std::vector<Batch> outs;
  outs.reserve((size_t)count);
  std::vector<int64_t> bytes((size_t)count, 0);   // of the selected chunks, per row group
  for (int g = 0; g < count; ++g)
    for (int ci : sel) bytes[(size_t)g] += f.row_groups[(size_t)(first + g)].columns[(size_t)ci].total_compressed_size;
  const std::vector<int> cuts = parquet_wave_cuts(bytes);
  for (size_t k = 0; k + 1 < cuts.size(); ++k) run_wave(ctx, f, first + cuts[k], first + cuts[k + 1], sel, outs);
  for (const Batch& b : outs)
    for (const Column& c : b.cols) {
      if (c.type == T_UTF8) ctx.stats.bytes_written_alg += (c.length + 1) * 4 + std::max<int64_t>(0, c.data_bytes);
      else if (c.type == T_BOOL) ctx.stats.bytes_written_alg += (c.length + 7) / 8;
      else ctx.stats.bytes_written_alg += c.length * c.width;
      if (c.validity) ctx.stats.bytes_written_alg += (c.length + 7) / 8;
    }
  return outs;
}

Batch parquet_read_row_group(Context& ctx, const PqFile& f, int row_group) {
  if (row_group < 0 || row_group >= (int)f.row_groups.size()) malformed("row group " + std::to_string(row_group) + " of " + std::to_string(f.row_groups.size()));
  std::vector<Batch> one = parquet_read_row_groups(ctx, f, row_group, 1);
  return std::move(one[0]);
}

}  // namespace chq
