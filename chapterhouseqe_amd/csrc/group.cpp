// group.cpp -- the batch-group filter: the one-launch path over the plans of group_plan.cpp, its routing and its detours
// (the per-batch loop and the two concat paths over group_concat.cpp).
#include "engine_internal.hpp"

#include <cstring>

namespace chq {

// =================================================================================================
// filter_records: filter_record over a group of batches that share one schema, in ONE launch.
//
// The reference hands the filter operator one 10 000-row batch at a time (physical_planner.rs:323); at that size a
// call is bounded by launch + read-back latency, not by HBM.  A group call keeps the per-batch semantics (one output
// batch per input batch, same rows, same order) but runs one chained-scan compaction over all tiles of all batches:
// tiles never straddle batches, a per-tile table carries the batch-local row range and the column pointers, the output
// of every column is one dense buffer and batch b's output is the slice between the inclusive prefixes of the last
// tiles of batches b-1 and b.
//
// Fast path: every column fixed-width (not Boolean / Utf8) and free of nulls, every batch >= 2 rows, predicate not
// literal-only, no static error.  Anything else -- and any data-dependent error -- takes the per-batch loop, which
// reports exactly what chq_filter_record would for the earliest failing batch.
// =================================================================================================
namespace {
// ---- the pieces of a group call ------------------------------------------------------------------------------------------
GroupOptions group_options(const Context& ctx) {
  return GroupOptions{ctx.opt_tile_kind, ctx.opt_group_mode, ctx.opt_group_bits, ctx.opt_fold_utf8, ctx.opt_group_fold, ctx.opt_group_chunk_bytes};
}

// batch b of a group as a view built from the flat arrays, with the schema of `first` (the head batch of a sub-group)
Batch lite_head(const Batch& first, const GroupLite& lite, size_t b) {
  Batch h = first;
  h.nrows = lite.rows[b];
  for (size_t i = 0; i < lite.ncols; ++i) {
    Column& c = h.cols[i];
    const size_t at = b * lite.ncols + i;
    c.owned.clear();
    c.offset = lite.offset[at]; c.length = lite.rows[b];
    c.values = c.type == T_BOOL ? lite.values0[at] : lite.values0[at] - (int64_t)(c.type == T_UTF8 ? 4 : c.width) * c.offset;
    c.data = lite.data[at]; c.data_bytes = -1;
    c.validity = lite.validity[at]; c.null_count = c.validity ? 1 : 0;   // (unknown count: may have nulls)
  }
  return h;
}

// filter_record over `cat`, the batches recs[b0, b1) back to back, with the output position of every batch reported by the
// device (split_bounds_kernel); the result where `out_on_device` says
JoinedGroup filter_joined(Context& ctx, const Batch& cat, const std::vector<Batch>& recs, size_t b0, size_t b1,
                          const chq_table_aliases* aliases, const Expr& expr, bool out_on_device) {
  SplitRequest split;
  int64_t at = 0;
  for (size_t b = b0; b < b1; ++b) { split.starts.push_back(at); at += recs[b].nrows; }
  split.starts.push_back(at);
  Batch res = filter_record(ctx, cat, plan_columns(cat, aliases), expr, &split);
  JoinedGroup g;
  g.joined = out_on_device ? std::move(res) : to_host(ctx, res);
  g.ends.assign(split.bounds.begin() + 1, split.bounds.end());
  return g;
}

// One group call.  `coalesce`: the caller wants ONE output batch (chq_filter_records_coalesced) -- the device join then
// declines a group it would have to cut, and the one-launch path does not split into short-string sub-groups.
struct GroupCall {
  Context& ctx;
  const GroupInput& gi;
  const chq_table_aliases* aliases;
  const Expr& expr;
  bool out_on_device, coalesce;
  const std::vector<Batch>& recs;   // batch 0 (schema, names); the others only after need_batches()
  const GroupLite& lite;            // every batch
  const size_t nb;

  GroupCall(Context& c, const GroupInput& g, const chq_table_aliases* a, const Expr& e, bool dev, bool co)
      : ctx(c), gi(g), aliases(a), expr(e), out_on_device(dev), coalesce(co), recs(g.batches), lite(g.lite), nb(g.lite.rows.size()) {}
  void need_batches() const { if (gi.materialise) gi.materialise(); }
  GroupResult per_batch_loop() const;
  GroupResult host_concat() const;
  GroupResult device_concat() const;
  // a concat path; a data-dependent error takes the per-batch loop, which reports the earliest failing batch's
  GroupResult concat(bool host) const {
    if (gi.head_only) return {};
    try {
      return host ? host_concat() : device_concat();
    } catch (const ChqError& e) {
      if (e.code == CHQ_ERR_OUT_OF_MEMORY || e.code == CHQ_ERR_DEVICE) throw;
      return per_batch_loop();
    }
  }
};

GroupResult GroupCall::per_batch_loop() const {
  if (gi.head_only) return {};
  need_batches();
  GroupResult r;
  chq_call_stats acc{};
  for (const Batch& rb : recs) {
    Batch dev = to_device(ctx, rb);
    Batch o = filter_record(ctx, dev, plan_columns(dev, aliases), expr);
    add_stats(acc, ctx.stats);
    r.per_batch.push_back(out_on_device ? std::move(o) : to_host(ctx, o));
  }
  ctx.stats = acc;
  return r;
}

// ---- host batches with Utf8 / Boolean / nullable columns: concatenated on the host while staging, filtered as ONE batch
// (every column kind is supported there), copied back once.  Chunks keep every Utf8 column below 1 GiB of bytes.
GroupResult GroupCall::host_concat() const {
  need_batches();
  std::vector<std::vector<int64_t>> bytes;
  for (size_t i = 0; i < recs[0].cols.size(); ++i) {
    if (recs[0].cols[i].type != T_UTF8) continue;
    bytes.emplace_back(nb, 0);
    for (size_t b = 0; b < nb; ++b) {
      const Column& c = recs[b].cols[i];
      if (c.values && c.length) { const int32_t* o = (const int32_t*)c.values + c.offset; bytes.back()[b] = (int64_t)o[c.length] - o[0]; }
    }
  }
  const std::vector<size_t> cuts = chunk_cuts(lite.rows, bytes, ctx.opt_group_chunk_bytes);
  GroupResult r;
  chq_call_stats acc{};
  for (size_t k = 0; k + 1 < cuts.size(); ++k) {
    Batch dev = to_device(ctx, concat_host_batches(recs, cuts[k], cuts[k + 1]));
    r.parts.push_back(filter_joined(ctx, dev, recs, cuts[k], cuts[k + 1], aliases, expr, out_on_device));
    add_stats(acc, ctx.stats);
  }
  ctx.stats = acc;
  return r;
}

// ---- device-resident batches with Utf8 / Boolean / nullable columns (the reference's own schema is Int32, Utf8, Float32:
// create_sample_data.rs:157-204): joined on the device by the concat kernels, filtered as ONE batch by the ordinary kernels.
// Chunks keep every Utf8 column below the int32 offset range.
GroupResult GroupCall::device_concat() const {
  need_batches();
  std::vector<int> utf8_cols;
  for (size_t i = 0; i < recs[0].cols.size(); ++i) if (recs[0].cols[i].type == T_UTF8) utf8_cols.push_back((int)i);
  PhaseTimer pt("device_concat_path");
  const std::vector<std::vector<int64_t>> ubytes = device_utf8_bytes(ctx, lite, utf8_cols);
  pt.mark("utf8_sizes");
  const std::vector<size_t> cuts = chunk_cuts(lite.rows, ubytes, ctx.opt_group_chunk_bytes);
  if (coalesce && cuts.size() > 2) throw ChqError{CHQ_ERR_ARROW_INVALID_ARGUMENT, "offset overflow: the joined Utf8 output of this group does not fit int32 offsets; use chq_filter_records"};
  GroupResult r;
  chq_call_stats acc{};
  for (size_t k = 0; k + 1 < cuts.size(); ++k) {
    const size_t b0 = cuts[k], b1 = cuts[k + 1];
    // (a chunk of one batch -- e.g. a 2 GB Utf8 column on its own -- is filtered in place: nothing to join)
    Batch cat = b1 - b0 == 1 ? to_device(ctx, recs[b0]) : concat_device_batches(ctx, recs, b0, b1, ubytes);
    pt.mark("join_launch");
    r.parts.push_back(filter_joined(ctx, cat, recs, b0, b1, aliases, expr, out_on_device));
    pt.mark("filter_record");
    add_stats(acc, ctx.stats);
  }
  ctx.stats = acc;
  return r;
}

GroupResult filter_group(Context& ctx, const GroupInput& gi, const chq_table_aliases* aliases, const Expr& expr,
                         bool out_on_device, bool coalesce);

// ---- stage 1: eligibility (plan_group, group_plan.hpp) over the flags, the row counts and batch 0's schema ---------------------
GroupPlan plan_group(const GroupCall& g) {
  std::vector<GroupCol> schema;
  for (const Column& c : g.recs[0].cols) schema.push_back(GroupCol{c.type, c.width});
  return plan_group(g.lite.flags, g.lite.rows, schema, !g.recs[0].on_device, group_options(g.ctx));
}

// The sizes of the folded Utf8 columns are read back from the device.  The read-back is queued when the call starts, before
// the predicate is typed, and awaited at the first get(): after the group table has been built (uniform_group: before it
// uploads its own table).
struct FoldSizesInFlight {
  Utf8Sizes z;
  bool done = false;
  std::vector<std::vector<int64_t>> bytes;   // of every folded Utf8 column per batch
  FoldSizes sizes;                           // and in all: `fits` false = long strings, or more than one output column can address
  const FoldSizes& get(Context& ctx, int64_t total_rows) {
    if (!done) { bytes = device_utf8_bytes_finish(ctx, z); sizes = fold_sizes(bytes, total_rows, ctx.opt_group_chunk_bytes); done = true; }
    return sizes;
  }
};

// ---- stage 2: a device group whose string columns all hold values of ONE length (the reference's sample strings, keys,
// hashes): fixed-width columns in disguise, as in filter_record -- one pass over every batch's offsets proves it, the group
// runs as a PLAIN group (value pointer of batch b = its data + its first offset) and every joined part gets back its Utf8
// columns (uniform_to_utf8).  False: a column does not qualify, or the plain group declined (e.g. a data-dependent error
// that the per-batch loop must attribute) -- the caller goes on as before.  `sizes`: the fold's size check.
bool uniform_group(const GroupCall& g, const GroupPlan& pl, FoldSizesInFlight& sizes, GroupResult* out) {
  Context& ctx = g.ctx;
  const GroupLite& lite = g.lite;
  const size_t nb = g.nb, ncols = lite.ncols, nu = pl.fold_utf8.size();
  for (int i : pl.fold_utf8) {
    bool bitmap = false;
    for (size_t b = 0; b < nb && !bitmap; ++b) bitmap = lite.validity[b * ncols + (size_t)i] != nullptr;
    if (!uniform_utf8_ok(bitmap, pl.total_rows, 1)) return false;
  }
  // (a group whose joined strings do not fit ONE output column is cut into sub-groups first: each comes back here)
  if (!sizes.get(ctx, pl.total_rows).fits) return false;
  std::vector<unsigned long long> h_in((nu + 1) * nb);
  for (size_t b = 0; b < nb; ++b) h_in[b] = (unsigned long long)lite.rows[b];
  for (size_t k = 0; k < nu; ++k)
    for (size_t b = 0; b < nb; ++b) h_in[(k + 1) * nb + b] = (unsigned long long)(uintptr_t)lite.values0[b * ncols + (size_t)pl.fold_utf8[k]];
  auto d_in = make_device_buffer(h_in.size() * 8 + 16, ctx.device);
  auto d_out = make_device_buffer(nu * nb * 12 + 16, ctx.device);
  check_hip(hipMemcpyAsync(d_in->ptr, h_in.data(), h_in.size() * 8, hipMemcpyHostToDevice, ctx.stream), "upload offsets table");
  check_hip(hipMemsetAsync(d_out->ptr, 0, nu * nb * 12, ctx.stream), "memset");
  for (size_t k = 0; k < nu; ++k) {
    Utf8UniformGroupParams up{(const unsigned long long*)d_in->ptr + (k + 1) * nb, (const long long*)d_in->ptr, (int64_t)nb, (int32_t*)d_out->ptr + 3 * k * nb};
    check_hip(launch_utf8_uniform_group(up, pl.max_rows, ctx.stream), "launch utf8_uniform_group_kernel");
  }
  std::vector<int32_t> h_out(nu * nb * 3);
  check_hip(hipMemcpyAsync(h_out.data(), d_out->ptr, h_out.size() * 4, hipMemcpyDeviceToHost, ctx.stream), "read back");
  check_hip(hipStreamSynchronize(ctx.stream), "hipStreamSynchronize");
  GroupInput sgi;   // the group with its string columns as FixedSizeBinary(L): pointers into the batches' bytes
  sgi.head_only = true;
  GroupLite& sub = sgi.lite = lite;
  Batch first = g.recs[0];
  for (size_t k = 0; k < nu; ++k) {
    const size_t i = (size_t)pl.fold_utf8[k];
    const int32_t L = h_out[3 * k * nb + 1];
    if (!uniform_utf8_ok(false, pl.total_rows, L)) return false;
    for (size_t b = 0; b < nb; ++b) {
      const int32_t* o = &h_out[3 * (k * nb + b)];
      if (o[0] || o[1] != L || o[2] < 0 || lite.data[b * ncols + i] == nullptr) return false;
      sub.values0[b * ncols + i] = lite.data[b * ncols + i] + o[2];
      sub.data[b * ncols + i] = nullptr;
      sub.offset[b * ncols + i] = 0;
    }
    Column& c = first.cols[i];
    c.type = T_FIXED_OPAQUE; c.format = "w:" + std::to_string(L); c.width = L;
  }
  for (uint8_t& f : sub.flags) f &= (uint8_t)~GroupLite::GL_NO_UTF8_DATA;
  sgi.batches.push_back(lite_head(first, sub, 0));
  GroupResult r = filter_group(ctx, sgi, g.aliases, g.expr, g.out_on_device, g.coalesce);
  if (r.parts.empty() || r.batches() != nb) return false;
  for (JoinedGroup& part : r.parts)
    for (int i : pl.fold_utf8) {
      Column& c = part.joined.cols[(size_t)i];
      c = uniform_to_utf8(ctx, std::move(c), g.recs[0].cols[(size_t)i], part.joined.nrows, g.out_on_device);
    }
  if (g.out_on_device) check_hip(hipStreamSynchronize(ctx.stream), "hipStreamSynchronize");
  ctx.stats.bytes_read_alg += (pl.total_rows + (int64_t)nb) * 4 * (int64_t)nu;
  *out = std::move(r);
  return true;
}

// ---- stage 3: the group table --------------------------------------------------------------------------------------------
struct GroupTable {
  std::vector<BufferPtr> staged;   // host groups: every column packed and uploaded
  Batch proto;                     // batch 0 with every column that has nulls in ANY batch marked nullable
  std::vector<BitCol> bit_cols;
  std::vector<int> launch_cols;
  FilterParams p{};
  GroupTiling tiling;              // wpb > 0: wave-granular mode
  GroupTableLayout lay;
};

// A host group packed column-wise into one staging block per column and uploaded with one copy each.  Returns where every
// batch's share lies in HBM, [batch][column] flat; the blocks are kept alive by `staged`.
std::vector<const uint8_t*> stage_host_group(const GroupCall& g, int64_t total_rows, std::vector<BufferPtr>& staged) {
  Context& ctx = g.ctx;
  const GroupLite& lite = g.lite;
  const size_t nb = g.nb, ncols = lite.ncols;
  std::vector<const uint8_t*> packed(nb * ncols);
  for (size_t i = 0; i < ncols; ++i) {
    const int64_t w = g.recs[0].cols[i].width;
    auto pack = make_host_buffer((size_t)(total_rows * w) + 16);   // recycled block: no page faults
    auto db = make_device_buffer((size_t)(total_rows * w) + 16, ctx.device);
    std::vector<int64_t> at(nb + 1, 0);
    for (size_t b = 0; b < nb; ++b) { at[b + 1] = at[b] + lite.rows[b] * w; packed[b * ncols + i] = (const uint8_t*)db->ptr + at[b]; }
    parallel_ranges(nb, (size_t)at[nb], [&](size_t k0, size_t k1) {
      for (size_t b = k0; b < k1; ++b) memcpy((uint8_t*)pack->ptr + at[b], lite.values0[b * ncols + i], (size_t)(lite.rows[b] * w));
    });
    check_hip(hipMemcpyAsync(db->ptr, pack->ptr, (size_t)at[nb], hipMemcpyHostToDevice, ctx.stream), "upload packed column");
    staged.push_back(db); staged.push_back(pack);
  }
  check_hip(hipStreamSynchronize(ctx.stream), "hipStreamSynchronize");
  return packed;
}

// `proto` (the program is lowered / pre-decoded against it: a ref that may be null must take the generic interpreter even if
// batch 0 happens to be null-free) and the bitmaps that ride along: the values of Boolean columns, the validity of every
// column with nulls in any batch -- from the flat per-batch arrays, no Batch objects, as in the null-free case
void derive_bit_cols(const GroupCall& g, GroupTable& t) {
  const GroupLite& lite = g.lite;
  const size_t ncols = lite.ncols;
  std::vector<char> col_nulls(ncols, 0);
  for (size_t b = 0; b < g.nb; ++b) {
    if (!(lite.flags[b] & GroupLite::GL_NULLS)) continue;
    for (size_t i = 0; i < ncols; ++i) if (lite.validity[b * ncols + i]) col_nulls[i] = 1;
  }
  for (size_t i = 0; i < ncols; ++i) {
    Column& pc = t.proto.cols[i];
    if (col_nulls[i]) { pc.validity = (const uint8_t*)pc.values; pc.null_count = 1; }   // (never read: a marker)
    else { pc.validity = nullptr; pc.null_count = 0; }
    if (pc.type == T_BOOL) t.bit_cols.push_back(BitCol{(int)i, false, 0});
    if (col_nulls[i]) t.bit_cols.push_back(BitCol{(int)i, true, 0});
  }
}

// input pointers, tiling and the table (in ctx.pinned_tbl); false: the group does not fit the one-launch path after all
bool build_group_table(const GroupCall& g, const GroupPlan& pl, const Lowered& lw, GroupTable& t) {
  Context& ctx = g.ctx;
  const std::vector<Batch>& recs = g.recs;
  ctx.stats = chq_call_stats{};
  ctx.stats.rows_in = pl.total_rows;
  // device batches are read where they lie (lite.values0), host batches where they were staged
  std::vector<const uint8_t*> packed;
  if (pl.host_in) packed = stage_host_group(g, pl.total_rows, t.staged);
  t.tiling = plan_tiling(lw.wide || lw.num_temps > 0, group_options(ctx), g.lite.rows, pl.total_rows, pl.max_rows);
  ensure_scratch(ctx, t.tiling.ntiles);
  t.proto = recs[0];
  if (pl.need_bits && t.tiling.wpb > 0) derive_bit_cols(g, t);   // (bitmaps of a ragged group: the layout declines, nothing to derive)
  // column order of the launch: the stashed predicate column goes last (see filter_record)
  for (size_t i = 0; i < recs[0].cols.size(); ++i) if (recs[0].cols[i].type != T_UTF8 && recs[0].cols[i].type != T_BOOL) t.launch_cols.push_back((int)i);
  pick_stash(t.p, ctx, lw, t.proto.cols, t.launch_cols, t.tiling.tile_kind);
  t.lay = layout_group_table(t.tiling, g.nb, lw.refs.size(), t.launch_cols.size(), pl.fold_utf8.size(), pl.need_bits, t.bit_cols);
  if (!t.lay.ok) return false;   // (e.g. bitmaps on a ragged group: joined on the device)
  // built in pinned memory, one upload
  ensure_pinned_table(ctx, t.lay.bytes_tbl + t.lay.bytes_idx + t.lay.bytes_cnt);
  write_group_table(t.lay, t.tiling, g.lite, pl.host_in ? packed.data() : g.lite.values0.data(), lw.refs, t.launch_cols, pl.fold_utf8,
                    t.bit_cols, (u64*)ctx.pinned_tbl.ptr);
  return true;
}

// ---- stage 4: ONE launch over the table, the joined outputs collected into `out` -------------------------------------------
// False: a data-dependent error was flagged (the per-batch loop reports the earliest failing batch, as the reference's
// loop would).  `fold_cap`: capacity of every folded Utf8 column's joined bytes.
bool launch_group(const GroupCall& g, const GroupPlan& pl, const Lowered& lw, GroupTable& t, const std::vector<int64_t>& fold_cap,
                  JoinedGroup& out) {
  Context& ctx = g.ctx;
  const std::vector<Batch>& recs = g.recs;
  const size_t nb = g.nb, ncols = recs[0].cols.size(), nu = pl.fold_utf8.size();
  const int64_t total_rows = pl.total_rows, ntiles = t.tiling.ntiles, wpb = t.tiling.wpb;
  const int tile_kind = t.tiling.tile_kind;
  FilterParams& p = t.p;
  PhaseTimer pt("filter_records (launch)");
  u64* h_cnt = (u64*)((uint8_t*)ctx.pinned_tbl.ptr + t.lay.bytes_tbl + t.lay.bytes_idx);
  auto d_tbl = make_device_buffer(t.lay.bytes_tbl + t.lay.bytes_idx + t.lay.bytes_cnt + 16, ctx.device);
  check_hip(hipMemcpyAsync(d_tbl->ptr, ctx.pinned_tbl.ptr, t.lay.bytes_tbl + t.lay.bytes_idx, hipMemcpyHostToDevice, ctx.stream), "upload group table");
  u64* d_cnt = (u64*)((uint8_t*)d_tbl->ptr + t.lay.bytes_tbl + t.lay.bytes_idx);
  Scratch* ds = dev_scratch(ctx);

  // ---- dense outputs ---------------------------------------------------------------------------------------
  std::vector<BufferPtr> dense(ncols), dense_data(ncols), fold_status;
  for (size_t i = 0; i < ncols; ++i) {
    if (recs[0].cols[i].type == T_UTF8 || recs[0].cols[i].type == T_BOOL) continue;
    dense[i] = make_device_buffer((size_t)(total_rows * recs[0].cols[i].width) + 16, ctx.device);
    ctx.stats.bytes_read_alg += total_rows * recs[0].cols[i].width;
  }
  BufferPtr g_sel, g_base;
  const int64_t nslots = pl.need_bits ? ntiles * kWavesPerTile[tile_kind] * (kWaveRows[tile_kind] / 64) : 0;
  if (pl.need_bits) {
    g_sel = make_device_buffer((size_t)(nslots + 8) * 8, ctx.device);
    g_base = make_device_buffer((size_t)(nslots + 8) * 8, ctx.device);
    p.sel_mask = (u64*)g_sel->ptr; p.grp_base = (u64*)g_base->ptr; p.group_bits_at = (int32_t)t.lay.bits_at; p.pb.group_bits_at = (int32_t)t.lay.bits_at;
  }
  for (size_t k = 0; k < nu; ++k) {   // Utf8 columns: joined offsets (from 0) and bytes, capacity = the input bytes
    const size_t i = (size_t)pl.fold_utf8[k];
    dense[i] = make_device_buffer((size_t)(total_rows + 2) * 4, ctx.device);
    dense_data[i] = make_device_buffer((size_t)fold_cap[k] + 64, ctx.device);
    auto st = make_device_buffer((size_t)(ntiles + 1) * 8, ctx.device);
    check_hip(hipMemsetAsync(st->ptr, 0, (size_t)(ntiles + 1) * 8, ctx.stream), "memset byte-scan status");
    fold_status.push_back(st);
    Utf8Fold& f = p.utf8[k];
    f.in_offsets = nullptr; f.in_data = nullptr;   // per batch, from the table
    f.out_offsets = (int32_t*)dense[i]->ptr; f.out_data = (uint8_t*)dense_data[i]->ptr;
    f.status = (u64*)st->ptr; f.total_bytes = &ds->fold_bytes[k];
    ctx.stats.bytes_read_alg += total_rows * 8;
  }
  p.n_utf8 = (int32_t)nu;
  p.nrows = ntiles * kTileRows[tile_kind];   // only locates the last tile; per-tile row ranges come from the table
  bind_scratch(p, ctx);
  fill_refs(p.pb, lw, t.proto, {});
  fill_outs(p, t.launch_cols, recs[0].cols, [](int) { return (const void*)nullptr; }, [&](int ci) { return dense[ci]->ptr; });   // (inputs: per batch, from the table)
  p.group = (const u64*)d_tbl->ptr; p.group_stride = (int64_t)t.lay.stride;
  p.group_wpb = (int32_t)wpb; p.group_nb = (int32_t)nb; p.group_batch_end = d_cnt;
  p.tile_begin = 0; p.tile_end = ntiles;
  clear_scratch(ctx, ntiles);
  kernel_span_begin(ctx);
  check_hip(launch_filter(p, tile_kind, true, (int)std::min<int64_t>(ntiles, grid_cap(ctx, tile_kind)), ctx.stream), "launch filter_fused_kernel (group)");
  kernel_span_end(ctx);
  ctx.stats.launches = 1; ctx.stats.tiles = ntiles;
  if (wpb == 0) {   // tile mode: the inclusive prefix at every batch's last tile
    GatherStatusParams gp{};
    gp.status = dev_status(ctx); gp.idx = (const int64_t*)((const uint8_t*)d_tbl->ptr + t.lay.bytes_tbl);
    gp.dst = d_cnt; gp.n = (int64_t)nb;
    check_hip(launch_gather_status(gp, ctx.stream), "launch gather_status_kernel");
    ctx.stats.launches = 2;
  }
  std::vector<BufferPtr> bit_out(t.bit_cols.size());
  const size_t bit_bytes = (size_t)(total_rows + 31) / 32 * 4 + 16;
  for (size_t q = 0; q < t.bit_cols.size(); ++q) {   // one joined bitmap per Boolean column / per column with nulls
    bit_out[q] = make_device_buffer(bit_bytes, ctx.device);
    check_hip(hipMemsetAsync(bit_out[q]->ptr, 0, bit_bytes, ctx.stream), "memset bits");
    BitCompactGroupParams bp{};
    bp.sel_mask = (const u64*)g_sel->ptr; bp.grp_base = (const u64*)g_base->ptr; bp.table = (const u64*)d_tbl->ptr; bp.stride = (int64_t)t.lay.stride;
    bp.word_ptr = (int32_t)t.bit_cols[q].word; bp.word_off = (int32_t)t.bit_cols[q].word + 1; bp.wpb = (int32_t)wpb; bp.nb = (int32_t)nb;
    bp.rows_per_wave = (int32_t)kWaveRows[tile_kind]; bp.out_bits = (uint32_t*)bit_out[q]->ptr;
    bp.zero_count = t.bit_cols[q].validity ? &ds->counters[q] : nullptr;
    check_hip(launch_bit_compact_group(bp, (int)std::min<int64_t>((wpb * (int64_t)nb + 3) / 4, (int64_t)ctx.num_cus * 8), ctx.stream), "launch bit_compact_group_kernel");
    ++ctx.stats.launches;
  }
  check_hip(hipMemcpyAsync(h_cnt, d_cnt, t.lay.bytes_cnt, hipMemcpyDeviceToHost, ctx.stream), "read back batch prefixes");
  pt.mark("alloc+launch");
  const Scratch* hs = read_scratch(ctx);
  pt.mark("kernel+readback");
  ctx.stats.kernel_ns += kernel_span_ns(ctx);
  if (hs->err != ERR_NONE) return false;
  const int64_t total = (int64_t)hs->total;
  ctx.stats.rows_out = total;
  std::vector<int64_t> out_bytes(ncols, 0);   // Utf8 columns: bytes of the joined output
  for (size_t k = 0; k < nu; ++k) {
    out_bytes[(size_t)pl.fold_utf8[k]] = (int64_t)hs->fold_bytes[k];
    ctx.stats.bytes_read_alg += (int64_t)hs->fold_bytes[k]; ctx.stats.bytes_written_alg += (total + 1) * 4 + (int64_t)hs->fold_bytes[k];
  }
  for (size_t i = 0; i < ncols; ++i) if (recs[0].cols[i].type != T_UTF8 && recs[0].cols[i].type != T_BOOL) ctx.stats.bytes_written_alg += total * recs[0].cols[i].width;

  // ---- the joined output columns: values (a Boolean column: its joined bitmap), Utf8 bytes, validity --------------------
  struct JoinedCol { BufferPtr values, data, validity; int64_t nulls = 0; };
  std::vector<JoinedCol> joined(ncols);
  for (size_t i = 0; i < ncols; ++i) { joined[i].values = dense[i]; joined[i].data = dense_data[i]; }
  for (size_t q = 0; q < t.bit_cols.size(); ++q) {
    JoinedCol& jc = joined[(size_t)t.bit_cols[q].col];
    if (!t.bit_cols[q].validity) jc.values = bit_out[q];
    else if (hs->counters[q] != 0) { jc.validity = bit_out[q]; jc.nulls = (int64_t)hs->counters[q]; }   // (arrow drops an all-valid null buffer)
  }
  if (!g.out_on_device) {   // host result: every joined buffer comes down once
    for (size_t i = 0; i < ncols; ++i) {
      const DType ty = recs[0].cols[i].type;
      auto down = [&](BufferPtr& b, size_t bytes) {
        if (!b) return;
        auto hb = make_host_buffer(bytes + 16);
        if (bytes) check_hip(hipMemcpyAsync(hb->ptr, b->ptr, bytes, hipMemcpyDeviceToHost, ctx.stream), "download joined column");
        b = hb;
      };
      down(joined[i].values, ty == T_UTF8 ? (size_t)(total + 1) * 4 : ty == T_BOOL ? (size_t)(total + 7) / 8 : (size_t)(total * recs[0].cols[i].width));
      down(joined[i].data, (size_t)out_bytes[i]);
      down(joined[i].validity, (size_t)(total + 7) / 8);
    }
    check_hip(hipStreamSynchronize(ctx.stream), "hipStreamSynchronize");
  }
  out.joined.on_device = g.out_on_device; out.joined.device_id = g.out_on_device ? ctx.device : -1;
  out.joined.nrows = total;
  for (size_t i = 0; i < ncols; ++i) {
    Column c = empty_like(recs[0].cols[i]);
    const JoinedCol& jc = joined[i];
    c.values = (const uint8_t*)jc.values->ptr; c.length = total; c.owned.push_back(jc.values);
    if (c.type == T_UTF8) { c.data = (const uint8_t*)jc.data->ptr; c.data_bytes = out_bytes[i]; c.owned.push_back(jc.data); }
    if (jc.validity) { c.validity = (const uint8_t*)jc.validity->ptr; c.null_count = jc.nulls; c.owned.push_back(jc.validity); }
    out.joined.cols.push_back(std::move(c));
  }
  out.ends.assign(h_cnt, h_cnt + nb);
  return true;
}

// Short strings whose JOINED output would not fit int32 offsets (the reference's batch size at config-5 scale: 10^5 batches,
// 8 GB of strings): consecutive sub-groups, each through the one-launch path -- no join on the device (2.7 ms per GiB
// chunk) and no Batch objects.  False: a sub-group of ONE batch (it would take the per-batch path: nothing gained -- e.g.
// ten 1 GB batches), or one that did not run as one launch.
bool split_short_strings(const GroupCall& g, const std::vector<std::vector<int64_t>>& fold_bytes, GroupResult* out) {
  const std::vector<size_t> cuts = chunk_cuts(g.lite.rows, fold_bytes, g.ctx.opt_group_chunk_bytes);
  if (!sub_groups_of_two(cuts)) return false;
  chq_call_stats acc{};
  GroupResult r;
  for (size_t k = 0; k + 1 < cuts.size(); ++k) {
    GroupInput sgi;
    sgi.head_only = true;
    sgi.lite = g.lite.slice(cuts[k], cuts[k + 1]);
    sgi.batches.push_back(lite_head(g.recs[0], g.lite, cuts[k]));
    GroupResult part = filter_group(g.ctx, sgi, g.aliases, g.expr, g.out_on_device, g.coalesce);
    add_stats(acc, g.ctx.stats);
    if (part.parts.size() != 1 || part.batches() != cuts[k + 1] - cuts[k]) return false;
    r.parts.push_back(std::move(part.parts[0]));
  }
  g.ctx.stats = acc;
  *out = std::move(r);
  return true;
}

GroupResult filter_group(Context& ctx, const GroupInput& gi, const chq_table_aliases* aliases, const Expr& expr,
                         bool out_on_device, bool coalesce) {
  const GroupCall g(ctx, gi, aliases, expr, out_on_device, coalesce);
  if (g.nb < 2 || g.recs[0].cols.empty()) return g.per_batch_loop();
  PhaseTimer pt("filter_records (one-launch path)");
  const GroupPlan pl = plan_group(g);
  if (pl.per_batch) return g.per_batch_loop();
  FoldSizesInFlight sizes;   // queued here, awaited behind the table
  if (pl.fold) sizes.z = device_utf8_bytes_issue(ctx, g.lite, pl.fold_utf8);
  pt.mark("eligibility+utf8_sizes");
  if (!pl.plain && !pl.fold) {   // joined first, on the host or on the device
    const bool host_case = pl.all_host && !out_on_device;
    if (!host_case && !pl.all_device) return g.per_batch_loop();
    try {
      if (!is_row_predicate(type_expr(expr, plan_columns(g.recs[0], aliases), g.recs[0].nrows, ctx.opt_enable_minus))) return g.per_batch_loop();
    } catch (const ChqError&) {
      return g.per_batch_loop();   // reports the first batch's (static) error
    }
    return g.concat(host_case);
  }
  // a foldable group that turns out not to fit the one-launch path is joined on the device instead
  auto other_path = [&]() -> GroupResult {
    if (!sizes.z.cols.empty()) check_hip(hipStreamSynchronize(ctx.stream), "hipStreamSynchronize");   // (the size gather reads back into pinned memory the next call reuses)
    return pl.fold ? g.concat(false) : g.per_batch_loop();
  };
  if (!pl.resident) return g.per_batch_loop();
  const std::vector<PlanColumn> pcols = plan_columns(g.recs[0], aliases);
  TypedExpr te = type_expr(expr, pcols, g.recs[0].nrows, ctx.opt_enable_minus);   // (a static error is thrown, not caught)
  if (!is_row_predicate(te)) return g.per_batch_loop();
  Lowered lw;
  try {
    lower_expr(te, te.root, pcols, lw);
  } catch (const ChqError& e) {
    if (e.code != CHQ_INTERNAL_PROGRAM_LIMIT) throw;
    return g.per_batch_loop();   // oversized predicate: every batch materialises its own temporaries
  }
  if (!lw.strs.empty()) return other_path();
  bool reads_utf8 = false;
  for (int r : lw.refs) reads_utf8 |= g.recs[0].cols[(size_t)r].type == T_UTF8;
  if (pl.fold && !reads_utf8 && ctx.opt_uniform_utf8_rows > 0 && pl.total_rows >= ctx.opt_uniform_utf8_rows) {
    GroupResult r;
    if (uniform_group(g, pl, sizes, &r)) return r;
  }
  // the predicate itself must not read a string column, and the wide / temporaries instantiation has no Utf8 form
  if (pl.fold && (reads_utf8 || lw.wide || lw.num_temps > 0)) return other_path();

  GroupTable t;
  if (!build_group_table(g, pl, lw, t)) return other_path();
  pt.mark("table");
  if (pl.fold && !sizes.get(ctx, pl.total_rows).fits) {
    GroupResult r;
    if (!coalesce && sizes.sizes.short_strings && split_short_strings(g, sizes.bytes, &r)) return r;
    return other_path();   // (long strings / too many bytes for one column: joined on the device)
  }
  pt.mark("utf8_sizes");
  GroupResult r;
  r.parts.emplace_back();
  if (!launch_group(g, pl, lw, t, sizes.sizes.cap, r.parts[0])) return g.per_batch_loop();
  return r;
}
}  // namespace

GroupResult filter_records(Context& ctx, const GroupInput& in, const chq_table_aliases* aliases, const Expr& expr,
                           bool out_on_device) {
  return filter_group(ctx, in, aliases, expr, out_on_device, false);
}

Batch filter_records_coalesced(Context& ctx, const GroupInput& in, const chq_table_aliases* aliases,
                               const Expr& expr, bool out_on_device, std::vector<int64_t>* rows_per_record) {
  if (in.batches.empty()) throw ChqError{CHQ_ERR_ARROW_INVALID_ARGUMENT, "no record batches to coalesce"};
  GroupResult r = filter_group(ctx, in, aliases, expr, out_on_device, true);
  std::vector<int64_t> rows;
  for (const JoinedGroup& part : r.parts)
    for (size_t b = 0; b < part.ends.size(); ++b) rows.push_back(part.ends[b] - (b ? part.ends[b - 1] : 0));
  for (const Batch& o : r.per_batch) rows.push_back(o.nrows);
  if (rows_per_record) *rows_per_record = rows;
  if (r.parts.size() == 1) return std::move(r.parts[0].joined);   // the joined batch IS the result
  // several host-joined parts, or the per-batch results: joined on the host, then moved where they are wanted
  const chq_call_stats st = ctx.stats;
  std::vector<Batch> host;
  for (JoinedGroup& part : r.parts) host.push_back(part.joined.on_device ? to_host(ctx, part.joined) : std::move(part.joined));
  for (Batch& o : r.per_batch) host.push_back(o.on_device ? to_host(ctx, o) : std::move(o));
  Batch cat = concat_host_batches(host, 0, host.size());
  Batch out = out_on_device ? to_device(ctx, cat) : std::move(cat);
  if (out_on_device) check_hip(hipStreamSynchronize(ctx.stream), "hipStreamSynchronize");
  ctx.stats = st;
  return out;
}

}  // namespace chq
