// engine_internal.hpp -- what the engine's own translation units (arrow_io.cpp, filter.cpp, group.cpp, group_concat.cpp,
// materialize.cpp, project.cpp) share with each other and with nobody else.  The interface for the rest of the library is engine.hpp.
#pragma once
#include <algorithm>

#include "engine.hpp"

namespace chq {

// ---- arrow_io.cpp: one column copied across (or within) memory spaces ----------------------------------------------------
enum class Dir { H2D, D2H, D2D, H2H, P2P };
// P2P: `ctx` is the DESTINATION context (buffers on its device, copies on its stream), `peer_device` the GPU `c` lives on
Column copy_column(Context& ctx, const Column& c, Dir dir, int peer_device = -1);

// ---- defined here: what the per-call host paths must be able to inline -----------------------------------------------------
inline void add_stats(chq_call_stats& acc, const chq_call_stats& s) {
  acc.rows_in += s.rows_in; acc.rows_out += s.rows_out; acc.tiles += s.tiles; acc.launches += s.launches;
  acc.bytes_read_alg += s.bytes_read_alg; acc.bytes_written_alg += s.bytes_written_alg; acc.kernel_ns += s.kernel_ns;
}

constexpr int kGridPerCu[3] = {1, 4, 4};   // (kTileRows: group_plan.hpp)

struct Scratch {   // header of ctx.small (device) and layout of ctx.pinned (host mirror)
  uint32_t ticket; uint32_t pad0;      // --- [0, kPerPass): re-cleared before every pass of a multi-pass filter
  unsigned long long total;
  uint32_t ticket2; uint32_t pad1;
  unsigned long long err;             // --- from here on: cleared once per call (errors accumulate over the passes)
  unsigned long long total_bytes;
  unsigned long long counters[24];
  int32_t utf8_ends[16];              // first / last input offset of each Utf8 column (output byte capacity)
  unsigned long long fold_bytes[MAX_FOLD_UTF8];   // output bytes of the Utf8 columns filtered inside the main kernel
};
constexpr size_t kPerPass = 24;
constexpr size_t kHeader = 512;       // status words start here
static_assert(sizeof(Scratch) <= kHeader, "scratch header");

inline void ensure_scratch(Context& ctx, int64_t ntiles) {
  if (!ctx.small || ctx.small_tiles < (size_t)ntiles + 64) {
    ctx.small_tiles = (size_t)ntiles + 64 + (size_t)ntiles / 4;
    ctx.small = make_device_buffer(kHeader + ctx.small_tiles * 8, ctx.device);
  }
  ctx.pinned.reserve(sizeof(Scratch), sizeof(Scratch), "hipHostMalloc");
}
inline Scratch* dev_scratch(Context& ctx) { return (Scratch*)ctx.small->ptr; }
inline u64* dev_status(Context& ctx) { return (u64*)((uint8_t*)ctx.small->ptr + kHeader); }
// The header into its pinned mirror, the stream synchronised.  (ensure_scratch may replace ctx.small: looked up per call.)
inline Scratch* read_scratch(Context& ctx) {
  Scratch* hs = (Scratch*)ctx.pinned.ptr;
  check_hip(hipMemcpyAsync(hs, dev_scratch(ctx), sizeof(Scratch), hipMemcpyDeviceToHost, ctx.stream), "read back");
  check_hip(hipStreamSynchronize(ctx.stream), "hipStreamSynchronize");
  return hs;
}
// header + the status words of `ntiles` tiles: cleared before a call's first chained-scan launch
inline void clear_scratch(Context& ctx, int64_t ntiles) {
  check_hip(hipMemsetAsync(dev_scratch(ctx), 0, kHeader + (size_t)(ntiles + 1) * 8, ctx.stream), "memset scratch + status");
}
template <class P>   // FilterParams, FusedParams
void bind_scratch(P& p, Context& ctx) {
  Scratch* ds = dev_scratch(ctx);
  p.status = dev_status(ctx); p.ticket = &ds->ticket; p.total = &ds->total; p.err = &ds->err;
}
// p.outs[k] copies launch column k from in(ci) to out(ci)
template <class In, class Out>
void fill_outs(FilterParams& p, const std::vector<int>& launch_cols, const std::vector<Column>& cols, In in, Out out) {
  p.n_out = 0;
  for (int ci : launch_cols) p.outs[p.n_out++] = OutCol{in(ci), out(ci), (uint32_t)cols[ci].width, 0};
}
inline int grid_cap(const Context& ctx, int tile_kind) { return ctx.num_cus * (ctx.opt_grid_per_cu > 0 ? (int)ctx.opt_grid_per_cu : kGridPerCu[tile_kind]); }

// launch(partial, grid, tail) over p's tiles.  Large batches: all complete tiles run in the instantiation without partial-tile
// code; the (single) incomplete tail tile in a second one-workgroup launch that continues the same chained scan.
template <class Params, class Launch>
void launch_tiles(Context& ctx, Params& p, int64_t rows, int64_t tile_rows, int64_t gcap, Launch&& launch) {
  const int64_t ntiles = (rows + tile_rows - 1) / tile_rows, nfull = rows / tile_rows;
  const bool split = rows >= ctx.opt_split_rows && nfull > 0;
  p.tile_begin = 0; p.tile_end = split ? nfull : ntiles;
  launch(!split, (int)std::min<int64_t>(p.tile_end, gcap), false);
  ++ctx.stats.launches;
  if (split && nfull < ntiles) {
    p.tile_begin = nfull; p.tile_end = ntiles;
    launch(true, 1, true);
    ++ctx.stats.launches;
  }
}

// A zero-row device column's buffers: 16 zeroed bytes of values (Utf8: offsets = {0}), for Utf8 a data buffer without bytes.
// Queued on the stream; the caller synchronises.
inline void give_empty_buffers(Context& ctx, Column& o) {
  auto vb = make_device_buffer(16, ctx.device);
  check_hip(hipMemsetAsync(vb->ptr, 0, 16, ctx.stream), "memset");
  o.values = (const uint8_t*)vb->ptr; o.owned.push_back(vb);
  if (o.type == T_UTF8) { auto db = make_device_buffer(16, ctx.device); o.data = (const uint8_t*)db->ptr; o.owned.push_back(db); }
}

// ---- filter.cpp: a lowered program and its launch ------------------------------------------------------------------------
void fill_refs(ProgramBlock& pb, const Lowered& lw, const Batch& rec, const std::vector<BufferPtr>& str_bufs);
BufferPtr upload_literal(Context& ctx, const std::string& s);
std::vector<BufferPtr> upload_strings(Context& ctx, const Lowered& lw);
[[noreturn]] void throw_device_error(unsigned long long stored);
int pick_tile_kind(const Context& ctx, const Lowered& lw, int64_t rows);
void pick_stash(FilterParams& p, const Context& ctx, const Lowered& lw, const std::vector<Column>& cols, std::vector<int>& launch_cols, int tile_kind);
// ---- materialize.cpp: expressions that do not fit one device program -------------------------------------------------------
bool lowers_alone(const TypedExpr& te, int node, const std::vector<PlanColumn>& wcols);
void fit_to_device(Context& ctx, const Batch& rec, const std::vector<PlanColumn>& pcols, const TypedExpr& original,
                   Batch& work, std::vector<PlanColumn>& wcols, TypedExpr& te);
// ---- filter.cpp: typing ------------------------------------------------------------------------------------------------------
TypedExpr typed(Context& ctx, const Batch& rec, const std::vector<PlanColumn>& pcols, const Expr& expr);
// `te` has a static error pending: a data-dependent error of its completed sub-trees (validate_roots, when there are rows), else it
[[noreturn]] void throw_pending(Context& ctx, const Batch& rec, const std::vector<PlanColumn>& pcols, const TypedExpr& te);
bool is_row_predicate(const TypedExpr& te);
Column empty_like(const Column& c);
// ---- filter.cpp: the uniform-length Utf8 rewrite -----------------------------------------------------------------------------
bool uniform_utf8_ok(bool may_hold_nulls, int64_t rows, int64_t L);
Column uniform_to_utf8(Context& ctx, Column&& fixed, const Column& like, int64_t rows, bool on_device);

// ---- group_concat.cpp: the batches of a group joined into one -----------------------------------------------------------------
// f(begin, end) over [0, n) on a few host threads when there is enough to copy (one thread moves ~10 GB/s, the PCIe
// link 55 GB/s: packing a group single-threaded would be the slowest step of a host-resident call)
template <class F>
void parallel_ranges(size_t n, size_t bytes, F&& f) {
  if (bytes < ((size_t)8 << 20) || n < 2) { f((size_t)0, n); return; }
  const size_t T = std::min<size_t>(std::min<size_t>(8, pool_width()), n);
  pool_ranges(n, (n + T - 1) / T, [&](size_t i0, size_t i1) { f(i0, i1); });
}
inline void ensure_pinned_table(Context& ctx, size_t bytes) {
  ctx.pinned_tbl.reserve(bytes, bytes + bytes / 4 + 4096, "hipHostMalloc (group table)");
}
Batch concat_host_batches(const std::vector<Batch>& recs, size_t b0, size_t b1);
Batch concat_device_batches(Context& ctx, const std::vector<Batch>& recs, size_t b0, size_t b1, const std::vector<std::vector<int64_t>>& utf8_bytes);
struct Utf8Sizes {   // the size gather of a group, in flight between device_utf8_bytes_issue and _finish
  std::vector<int> cols;
  size_t nb = 0;
  BufferPtr d_tbl;
  int32_t* h_ends = nullptr;   // [cols][2 nb] in ctx.pinned_sizes
};
Utf8Sizes device_utf8_bytes_issue(Context& ctx, const GroupLite& lite, const std::vector<int>& utf8_cols);
std::vector<std::vector<int64_t>> device_utf8_bytes_finish(Context& ctx, const Utf8Sizes& z);
std::vector<std::vector<int64_t>> device_utf8_bytes(Context& ctx, const GroupLite& lite, const std::vector<int>& utf8_cols);

// ---- project.cpp: typed trees evaluated densely over a batch, one column per expression ------------------------------------
std::vector<Column> evaluate_dense(Context& ctx, const Batch& rec, const std::vector<PlanColumn>& pcols, const std::vector<const TypedExpr*>& exprs);

}  // namespace chq
