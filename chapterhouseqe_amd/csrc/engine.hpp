// engine.hpp -- context, device memory, Arrow C Data import/export and the record-level operations.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <memory>
#include <mutex>
#include <chrono>
#include <functional>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/chq.h"
#include "device_program.h"
#include "typed_ops.h"
#include "like_device.h"
#include "strfn_device.h"
#include "cast_device.h"
#include "plan.hpp"
#include "group_plan.hpp"

namespace chq {

// kernels.hip
hipError_t launch_filter(const FilterParams& p, int tile_kind, bool partial, int grid, hipStream_t stream);
hipError_t launch_filter_project(const FusedParams& p, int tile_kind, int grid, hipStream_t stream);
hipError_t launch_project(const ProjectParams& p, int tile_kind, bool partial, int grid, hipStream_t stream);
hipError_t launch_bit_compact(const BitCompactParams& p, int grid, hipStream_t stream);
hipError_t launch_bit_compact_group(const BitCompactGroupParams& p, int grid, hipStream_t stream);
hipError_t launch_cmp128(const Cmp128Params& p, hipStream_t stream);
hipError_t launch_utf8_to_bool(const Utf8ToBoolParams& p, hipStream_t stream);
hipError_t launch_is_null(const IsNullParams& p, hipStream_t stream);
hipError_t launch_like(const LikeParams& p, hipStream_t stream);   // like.hip
// strfn.hip
hipError_t launch_strfn_bytemap(const StrByteMapParams& p, hipStream_t stream);
hipError_t launch_strfn_rebase(const StrRebaseParams& p, hipStream_t stream);
hipError_t launch_strfn_rows(const StrRowsParams& p, hipStream_t stream);
hipError_t launch_offsets_scan(const OffsetsScanParams& p, hipStream_t stream);   // scan.hip: 3 launches; tile_sums: ntiles + 1 words
hipError_t launch_strfn_gather(const StrGatherParams& p, hipStream_t stream);
// case.hip
hipError_t launch_case_masks(const CaseMasksParams& p, hipStream_t stream);
hipError_t launch_case_and(const CaseAndParams& p, hipStream_t stream);
hipError_t launch_case_select_bool(const CaseSelectParams& p, hipStream_t stream);
hipError_t launch_case_select_fixed(const CaseSelectParams& p, hipStream_t stream);
hipError_t launch_case_rows(const CaseSelectParams& p, hipStream_t stream);
hipError_t launch_case_gather(const CaseSelectParams& p, hipStream_t stream);
// cast.hip
hipError_t launch_cast_fixed(const CastFixedParams& p, hipStream_t stream);
hipError_t launch_cast_parse(const CastParseParams& p, hipStream_t stream);
hipError_t launch_cast_len(const CastPrintParams& p, hipStream_t stream);
hipError_t launch_cast_write(const CastPrintParams& p, hipStream_t stream);
// temporal.hip
hipError_t launch_temporal_part(const TemporalParams& p, hipStream_t stream);
hipError_t launch_temporal_trunc(const TemporalParams& p, hipStream_t stream);
hipError_t launch_utf8_uniform(const Utf8UniformParams& p, hipStream_t stream);
hipError_t launch_iota_offsets(const IotaOffsetsParams& p, hipStream_t stream);
hipError_t launch_count_bits(const uint8_t* in, int64_t bit_offset, int64_t nbits, unsigned long long* out, hipStream_t stream);
hipError_t launch_utf8_uniform_group(const Utf8UniformGroupParams& p, int64_t max_rows, hipStream_t stream);
hipError_t launch_utf8_filter(const Utf8Params& p, int grid, hipStream_t stream);
hipError_t launch_gather_i32(const GatherParams& p, hipStream_t stream);
hipError_t launch_gather_status(const GatherStatusParams& p, hipStream_t stream);
hipError_t launch_split_bounds(const SplitBoundsParams& p, hipStream_t stream);
hipError_t launch_utf8_offsets(const Utf8Params& p, int grid, hipStream_t stream);
hipError_t launch_utf8_copy(const Utf8Params& p, int grid, hipStream_t stream);
hipError_t launch_concat(const ConcatParams& p, int kind, int grid, hipStream_t stream);   // kind: 0 fixed, 1 ends, 2 utf8, 3 bits

// ---- memory ---------------------------------------------------------------------------------------
// Process-wide caching allocator for HBM (outlives contexts: Arrow release callbacks may run after the
// context that produced a batch is gone).  Blocks are recycled by size class; nothing is returned to
// HIP until trim().
class DevicePool {
 public:
  static DevicePool& instance();
  void* alloc(size_t bytes, int device, size_t* cap);
  void free(void* p, size_t cap, int device);
  void trim();
 private:
  std::mutex mu_;
  std::unordered_map<uint64_t, std::vector<void*>> free_;   // (size class, device) -> cached blocks
};

// The same for host memory handed out as result buffers.  A fresh host allocation costs a page fault per 4 KiB the
// first time the D2H copy touches it (measured: 8.8 GB/s instead of 55 GB/s); recycled blocks are already mapped.
// Only blocks >= 1 MiB are cached, up to `limit` bytes in total; the rest goes straight back to the C allocator.
class HostPool {
 public:
  static HostPool& instance();
  void* alloc(size_t bytes, size_t* cap);
  void free(void* p, size_t cap);
  void trim();
  void set_limit(size_t bytes);
 private:
  std::mutex mu_;
  std::unordered_map<size_t, std::vector<void*>> free_;
  size_t cached_ = 0;
  size_t limit_ = (size_t)8 << 30;
};

// One allocation (device or host) owned by an exported batch.
struct Buffer {
  void* ptr = nullptr;
  size_t bytes = 0;
  size_t cap = 0;          // size class the pool handed out
  int device_id = 0;
  bool device = false;
  ~Buffer();
  Buffer() = default;
  Buffer(const Buffer&) = delete;
  Buffer& operator=(const Buffer&) = delete;
};
using BufferPtr = std::shared_ptr<Buffer>;
BufferPtr make_device_buffer(size_t bytes, int device);
BufferPtr make_host_buffer(size_t bytes);

// ---- batches ----------------------------------------------------------------------------------------
// A column as stored (device or host pointers), Arrow layout.
struct Column {
  std::string name;
  std::string format;      // Arrow C format string
  DType type = T_FIXED_OPAQUE;
  int width = 0;           // bytes per value for fixed-width types
  bool nullable = false;   // schema flag
  int64_t length = 0;
  int64_t null_count = 0;
  int64_t offset = 0;      // Arrow slice offset (elements)
  const uint8_t* validity = nullptr;
  const uint8_t* values = nullptr;   // fixed: values buffer; bool: bitmap; utf8: int32 offsets buffer
  const uint8_t* data = nullptr;     // utf8 bytes
  int64_t data_bytes = -1;           // utf8: bytes the offsets of rows [offset, offset+length] span, when whoever built the column knew (else -1)
  std::vector<BufferPtr> owned;      // keeps staged / produced buffers alive

  // derived views (element 0 = first logical row)
  const void* values0() const;       // fixed: values + offset*width; utf8: offsets + offset
  int64_t bool_bit_offset() const { return offset; }
  int64_t validity_bit_offset() const { return offset; }
  // the bitmap when it may hold nulls (null_count unknown or positive), else nullptr: what a kernel is given
  const uint8_t* live_validity() const { return (validity && null_count != 0) ? validity : nullptr; }
};

struct Batch {
  int64_t nrows = 0;
  bool on_device = false;
  int device_id = 0;
  std::vector<Column> cols;
};

// ---- context ------------------------------------------------------------------------------------------
void check_hip(hipError_t e, const char* what);
// A grow-only block of pinned host memory (staging that the copy engine reads and writes directly).  Every user has its own
// capacity formula: `reserve` allocates `capacity` bytes when the block holds fewer than `need` (the old contents are lost).
struct PinnedBlock {
  void* ptr = nullptr;
  size_t bytes = 0;
  void reserve(size_t need, size_t capacity, const char* what) {
    if (bytes >= need) return;
    if (ptr) (void)hipHostFree(ptr);
    ptr = nullptr; bytes = 0;
    check_hip(hipHostMalloc(&ptr, capacity, hipHostMallocDefault), what);
    bytes = capacity;
  }
  PinnedBlock() = default;
  PinnedBlock(const PinnedBlock&) = delete;
  PinnedBlock& operator=(const PinnedBlock&) = delete;
  ~PinnedBlock() { if (ptr) (void)hipHostFree(ptr); }
};

struct Context {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  int num_cus = 0;
  std::string last_error;
  chq_call_stats stats{};
  // launches and algorithmic bytes of the temporal kernels (temporal.hip) since the current C ABI entry began: they run while an
  // expression is fitted, before the operator resets `stats`, so they are kept apart and added by chq_ctx_last_stats
  chq_call_stats typed_stats{};
  // options
  int64_t opt_tile_kind = -1;       // -1 auto
  bool opt_enable_minus = false;
  bool opt_time_kernels = false;
  int64_t opt_large_host = 1;       // host batches of opt_large_host_rows rows or more: chunked, uploads and downloads overlapped
  int64_t opt_large_host_rows = 8 << 20;
  int64_t opt_large_host_chunk = 0;  // rows per chunk (0: about 64 MB of input)
  int64_t opt_group_bits = 1;       // wave-packed device groups with validity bitmaps / Boolean columns take the one-launch path (0: joined first)
  int64_t opt_uniform_utf8_rows = 1 << 24;   // batches from this size on (below it the extra pass and its read-back cost more than the copy saves): Utf8 columns whose values all have one length are filtered as fixed-width columns (0: never)
  int64_t opt_parquet_page_rows = 65536;   // chq_record_to_parquet: rows per data page (multiples of 4096; at most 64 pages per chunk)
  int64_t opt_snappy_blocks = 1;           // Parquet scan: snappy pages of 3+ blocks of 64 KiB are inflated block by block (0: one wave per page; 2: the blocks give up -- tests)
  int64_t opt_group_fold = 1;       // device-resident groups with short-string Utf8 columns: filtered straight out of the batches (0: joined first)
  int64_t opt_fold_utf8 = 1;        // short-string Utf8 columns are filtered inside filter_fused_kernel (0: always the separate Utf8 pass)
  int64_t opt_stash = -1;           // predicate input columns kept in LDS between the filter kernel's phases: -1 = as many as the tile kind has slots
  int64_t opt_fuse = 1;             // chq_filter_project_record's single-pass kernel: 0 never, 1 when it moves clearly fewer bytes, 2 whenever possible
  int64_t opt_grid_per_cu = 0;
  int64_t opt_split_rows = 1 << 20;   // batches at least this long run their complete tiles in the FULL-only kernels
  int64_t opt_group_chunk_bytes = 1ll << 30;   // host-concatenated groups: Utf8 bytes per column and chunk (int32 offsets)
  int64_t opt_group_mode = 0;       // batch-group launch: 0 auto, 1 force per-tile table, 2 force wave-granular packing
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  // Parquet scan: the columns of a row group decode side by side (their per-page kernels are latency-bound, one wave per
  // page); created on first use, joined back into `stream` before anything is read back
  static constexpr int kAuxStreams = 13;    // twelve for kernels + kCopyStream for uploads
  // Uploads of the Parquet scan go through a stream of their own.  A copy from pageable host memory keeps the calling
  // thread until the copy has RUN, and on a column's kernel stream it runs behind every kernel queued there: with a slow
  // page decode on that stream (a 70 ms inflate) the host sat in the next upload instead of issuing the other columns' work,
  // and the columns decoded one after the other.  On the copy stream an upload waits for earlier uploads only; the column's
  // stream waits for it through an event.
  static constexpr int kCopyStream = 12;
  static constexpr int kKernelStreams = 12;
  std::vector<hipEvent_t> upload_events;    // pool: one per column in flight (parquet_scan.cpp)
  hipStream_t aux[kAuxStreams] = {};
  hipEvent_t aux_fork = nullptr, aux_join[kAuxStreams] = {};
  bool aux_ready = false;           // every auxiliary stream and event exists (ensure_aux_streams)
  // reusable device scratch
  BufferPtr small;          // [Scratch header (512 B)] [status words of the chained scan]: cleared by ONE memset per call
  size_t small_tiles = 0;   // status words the block has room for
  PinnedBlock pinned;                      // pinned host staging for small read-backs (the Scratch header)
  PinnedBlock pinned_tbl;                  // pinned staging of a batch-group launch (tile table, per-batch prefixes)
  PinnedBlock pinned_sizes;                // pinned staging of the Utf8 size gather of a group (in flight while the table is built)
  PinnedBlock pinned_io;                   // pinned staging of the small host-batch path: [inputs | outputs]
  BufferPtr dev_io;                        // its device twin
  bool opt_small_host = true;              // host batches up to a few MB: one upload, one download, one synchronisation

  ~Context();
};

// the auxiliary streams of a context: created on first use (one site), forked off / joined back into ctx.stream with events
void ensure_aux_streams(Context& ctx);
void fork_aux_streams(Context& ctx);
void join_aux_streams(Context& ctx);
// `time_kernels`: one span of ctx.stream between the context's two events (created on first use).  kernel_span_ns -- once
// the stream has been synchronised past kernel_span_end -- is its length; callers add it to stats.kernel_ns.  Off: 0.
void kernel_span_begin(Context& ctx);
void kernel_span_end(Context& ctx);
int64_t kernel_span_ns(Context& ctx);

// Arrow C Data Interface <-> Batch (`copy_only`: see parse_arrow_format)
Batch import_batch(const ArrowDeviceArray* rec, const ArrowSchema* schema, bool copy_only = false);
// `sync_event`: optional event the consumer must wait on; the exported array owns it (destroyed on release)
void export_batch(Batch&& b, int device_type, ArrowDeviceArray* out, ArrowSchema* out_schema, hipEvent_t sync_event = nullptr);
void export_single_column(Column&& c, bool on_device, int device_id, ArrowDeviceArray* out, ArrowSchema* out_schema);
// the caller's output structs read as released (either may be null)
void mark_released(ArrowDeviceArray* out, ArrowSchema* out_schema);
// (count_nulls_host: group_plan.hpp)

Batch to_device(Context& ctx, const Batch& b);   // stage host batch into HBM (no-op view when already there)
Batch to_host(Context& ctx, const Batch& b);
// device batch on src's GPU -> fresh buffers on dst's GPU (hipMemcpyPeerAsync on dst's stream); *event_out receives an
// event recorded behind the last copy (the caller owns it)
Batch copy_to_peer(Context& src, Context& dst, const Batch& b, hipEvent_t* event_out);

// the record-level operations (throw ChqError)
// `split`: optional input-row positions (ascending); on return bounds[i] = selected rows before starts[i], i.e. where the
// output of a batch that was concatenated into `rec_dev` at row starts[i] begins
struct SplitRequest { std::vector<int64_t> starts; std::vector<int64_t> bounds; };
Batch filter_record(Context& ctx, const Batch& rec_dev, const std::vector<PlanColumn>& pcols, const Expr& expr,
                    SplitRequest* split = nullptr);
// A small host batch, host result: columns staged through one pinned block each way (one H2D, one D2H, one stream
// synchronisation).  False = outside its scope or an error was flagged: take the general path.
bool filter_record_small_host(Context& ctx, const Batch& rec_host, const chq_table_aliases* aliases, const Expr& expr, Batch* result);
bool filter_record_large_host(Context& ctx, const Batch& rec_host, const chq_table_aliases* aliases, const Expr& expr, Batch* result);
// GroupLite, the per-batch facts of a group in flat arrays: group_plan.hpp
// The joined result of a group call, or of consecutive batches of it: ONE batch holding every surviving row in input order
// (columns as the producing path built them, buffers kept alive by Column::owned) and the exclusive end row of every input
// batch it covers.  chq_filter_records cuts it into per-batch Arrow structs from one block (export_group);
// chq_filter_records_coalesced hands the batch on whole.
struct JoinedGroup {
  Batch joined;
  std::vector<int64_t> ends;
};
// What a group call returns: consecutive joined parts that cover the batches in order, or (no parts) the per-batch results
// of the per-batch loop.
struct GroupResult {
  std::vector<JoinedGroup> parts;
  std::vector<Batch> per_batch;
  size_t batches() const {   // input batches the result covers
    size_t n = per_batch.size();
    for (const JoinedGroup& p : parts) n += p.ends.size();
    return n;
  }
};
// The batches of a group call: `lite` describes every batch, `batches` holds batch 0 (schema, names) and -- once
// `materialise` (imports every batch; idempotent; empty: nothing left to import) has run -- the others.  The one-launch path
// works from `lite` alone: 10^4 Batch objects it never looks at cost more to build and free than the rest of the call's
// host work.  `head_only`: a sub-group cut out of a larger call; the other batches cannot be had, and the paths that read
// Batch objects decline it -- no parts, no per-batch results -- so that the caller goes on with the whole group.
struct GroupInput {
  std::vector<Batch> batches;
  GroupLite lite;
  std::function<void()> materialise;
  bool head_only = false;
};
// arrow_io.cpp: the Arrow structs of a group.  import_group fills `gi` from `n_records` >= 1 non-null records of one schema;
// export_group writes one output per batch `g` covers, all of them or -- it throws -- none (the structs left released).
void import_group(int n_records, const ArrowDeviceArray* const* recs, const ArrowSchema* schema, int device, GroupInput& gi);
void export_group(JoinedGroup&& g, int device_type, ArrowDeviceArray* outs, ArrowSchema* out_schemas);
// one launch for a group of same-schema batches (host or device resident); outputs where `out_on_device` says
GroupResult filter_records(Context& ctx, const GroupInput& in, const chq_table_aliases* aliases, const Expr& expr,
                           bool out_on_device);
// the same, but ONE output batch holding every surviving row in input order (+ surviving rows per input batch)
Batch filter_records_coalesced(Context& ctx, const GroupInput& in, const chq_table_aliases* aliases,
                               const Expr& expr, bool out_on_device, std::vector<int64_t>* rows_per_record);
Batch project_record(Context& ctx, const std::vector<chq_select_item>& fields, const Batch& rec_dev,
                     const std::vector<PlanColumn>& pcols);
// filter_record + project_record in one kernel pass; false = outside its scope (or an error was flagged): run the two steps
bool filter_project_fused(Context& ctx, const Batch& rec_dev, const std::vector<PlanColumn>& pcols, const Expr& pred,
                          const std::vector<chq_select_item>& fields, Batch* result);
// project_record for a host batch with a host result: pass-through columns never cross PCIe; false = general path
bool project_record_host(Context& ctx, const std::vector<chq_select_item>& fields, const Batch& rec_host,
                         const chq_table_aliases* aliases, Batch* result);
Column compute_value(Context& ctx, const Batch& rec_dev, const std::vector<PlanColumn>& pcols, const Expr& expr,
                     bool* is_scalar);

std::vector<PlanColumn> plan_columns(const Batch& b, const chq_table_aliases* aliases);

// Arrow C format string -> column kind and byte width (throws CHQ_ERR_NOT_SUPPORTED outside the build's scope).
// The kernels move values of 1, 2, 4, 8 and 16 bytes; `copy_only` is for the callers that move a column's bytes and launch no
// kernel on its values (staging, peer copy, Arrow IPC): they take FixedSizeBinary of every width.
void parse_arrow_format(const char* format, DType* type, int* width, bool copy_only = false);

// A few persistent host threads for per-batch bookkeeping of large groups (importing / exporting 10^4..10^5 Arrow structs,
// building pointer tables): f(t) for t in [0, tasks), the caller takes part, the first exception is rethrown.  Creating
// threads per call cost more than the work at 12 500 batches (0.5 of 0.85 ms).  Re-entrant calls run inline.
void pool_run(unsigned tasks, const std::function<void(unsigned)>& f);
unsigned pool_width();   // threads that take part (including the caller)
// f(i0, i1) over [0, n) split into at most pool_width() ranges of at least `grain` items
void pool_ranges(size_t n, size_t grain, const std::function<void(size_t, size_t)>& f);
// f(i) for i in [0, n) on those threads when the group is large: importing / exporting 10^5 Arrow structs one after the
// other (~0.3 + 0.4 us each) used to be 93 % of a group call (round 1).  The first error, if any, is rethrown.
template <class F>
void for_each_parallel(int n, F&& f) {
  if (n < 2048) { for (int i = 0; i < n; ++i) f(i); return; }
  pool_ranges((size_t)n, 1024, [&](size_t i0, size_t i1) { for (size_t i = i0; i < i1; ++i) f((int)i); });
}

// Wall-clock phases of one call, printed to stderr when the environment has CHQ_TIMING=1 (development aid; off: one getenv
// per process).
struct PhaseTimer {
  const char* what; bool on; std::chrono::steady_clock::time_point t0, last; std::string line;
  explicit PhaseTimer(const char* w);
  void mark(const char* phase);
  ~PhaseTimer();
};

// ---- Arrow IPC stream with the body in HBM (ipc.cpp) ------------------------------------------------------------------
struct IpcMessage {
  std::vector<uint8_t> header;   // host: Schema message + the RecordBatch message's framing and metadata
  BufferPtr body;                // every Arrow buffer, 64-byte aligned, back to back
  int64_t body_len = 0;
  bool body_on_device = true;
  BufferPtr keep;
};
IpcMessage record_to_ipc(Context& ctx, const Batch& rec_dev, bool body_on_device);
// `body` null: the body follows the batch message inside `stream` (a complete host stream)
std::string describe_ipc(const uint8_t* stream, int64_t stream_len);   // host only
Batch record_from_ipc(Context& ctx, const uint8_t* stream, int64_t stream_len, const void* body, int64_t body_len,
                      bool body_on_device, bool out_on_device);

// host-only: result type / flags and the lowered device program of `expr` over a schema (text); throws the static error
std::string describe_plan(const ArrowSchema* schema, const chq_table_aliases* aliases, const Expr& expr, int64_t nrows,
                          bool enable_minus);

}  // namespace chq
