// group.cpp -- the batch-group filter: eligibility, host and device concatenation, the group table, the one-launch path and
// its detours.
#include "engine_internal.hpp"

#include <atomic>
#include <cstring>
#include <mutex>

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
// f(begin, end) over [0, n) on a few host threads when there is enough to copy (one thread moves ~10 GB/s, the PCIe
// link 55 GB/s: packing a group single-threaded would be the slowest step of a host-resident call)
template <class F>
void parallel_ranges(size_t n, size_t bytes, F&& f) {
  if (bytes < ((size_t)8 << 20) || n < 2) { f((size_t)0, n); return; }
  const size_t T = std::min<size_t>(std::min<size_t>(8, pool_width()), n);
  pool_ranges(n, (n + T - 1) / T, [&](size_t i0, size_t i1) { f(i0, i1); });
}

// ---- host-side concatenation of a group (general column kinds) -----------------------------------------------
// append n bits of src starting at bit src_bit (src == nullptr: ones) to dst at bit dst_bit; dst is zero-filled and has
// 8 spare bytes behind its last bit
void append_bits(uint8_t* dst, int64_t dst_bit, const uint8_t* src, int64_t src_bit, int64_t n) {
  while (n > 0) {
    const int k = (int)std::min<int64_t>(n, 56);
    uint64_t v;
    if (src) {
      const int sh = (int)(src_bit & 7);
      const int nbytes = (sh + k + 7) / 8;
      uint64_t raw = 0;
      memcpy(&raw, src + (src_bit >> 3), (size_t)nbytes);
      v = (raw >> sh) & ((1ULL << k) - 1ULL);
    } else {
      v = (1ULL << k) - 1ULL;
    }
    const int dsh = (int)(dst_bit & 7);
    uint64_t cur;
    uint8_t* dp = dst + (dst_bit >> 3);
    memcpy(&cur, dp, 8);
    cur |= v << dsh;                       // k + dsh <= 63
    memcpy(dp, &cur, 8);
    dst_bit += k; src_bit += k; n -= k;
  }
}

// one host batch holding the rows of recs[b0, b1) back to back (buffers from the recycling host pool)
Batch concat_host_batches(const std::vector<Batch>& recs, size_t b0, size_t b1) {
  Batch cat;
  cat.on_device = false; cat.device_id = -1;
  int64_t total = 0;
  for (size_t b = b0; b < b1; ++b) total += recs[b].nrows;
  cat.nrows = total;
  const size_t ncols = recs[b0].cols.size();
  for (size_t i = 0; i < ncols; ++i) {
    const Column& c0 = recs[b0].cols[i];
    Column o = empty_like(c0);
    o.length = total;
    bool any_nulls = false;
    for (size_t b = b0; b < b1; ++b) { const Column& c = recs[b].cols[i]; any_nulls |= c.validity && c.null_count != 0; }
    if (any_nulls) {
      auto vb = make_host_buffer((size_t)(total + 7) / 8 + 16);
      memset(vb->ptr, 0, (size_t)(total + 7) / 8 + 16);
      int64_t at = 0, nulls = 0;
      for (size_t b = b0; b < b1; ++b) {
        const Column& c = recs[b].cols[i];
        const bool has = c.validity && c.null_count != 0;
        append_bits((uint8_t*)vb->ptr, at, has ? c.validity : nullptr, c.offset, c.length);
        if (has) nulls += c.null_count > 0 ? c.null_count : count_nulls_host(c.validity, c.offset, c.length);
        at += c.length;
      }
      o.validity = (const uint8_t*)vb->ptr; o.null_count = nulls; o.owned.push_back(vb);
    }
    if (c0.type == T_BOOL) {
      auto vb = make_host_buffer((size_t)(total + 7) / 8 + 16);
      memset(vb->ptr, 0, (size_t)(total + 7) / 8 + 16);
      int64_t at = 0;
      for (size_t b = b0; b < b1; ++b) { const Column& c = recs[b].cols[i]; append_bits((uint8_t*)vb->ptr, at, c.values, c.offset, c.length); at += c.length; }
      o.values = (const uint8_t*)vb->ptr; o.owned.push_back(vb);
    } else if (c0.type == T_UTF8) {
      const size_t n = b1 - b0;
      std::vector<int64_t> row_at(n + 1, 0), byte_at(n + 1, 0);
      for (size_t k = 0; k < n; ++k) {
        const Column& c = recs[b0 + k].cols[i];
        int64_t nbytes = 0;
        if (c.values && c.length) { const int32_t* offs = (const int32_t*)c.values + c.offset; nbytes = (int64_t)offs[c.length] - offs[0]; }
        row_at[k + 1] = row_at[k] + c.length; byte_at[k + 1] = byte_at[k] + nbytes;
      }
      // Arrow Utf8 offsets are int32: a joined column of 2 GiB or more cannot be represented (arrow's concat reports
      // an offset overflow; wrapping silently would hand out negative offsets)
      if (byte_at[n] > (int64_t)INT32_MAX)
        throw ChqError{CHQ_ERR_ARROW_INVALID_ARGUMENT, "offset overflow: Utf8 column '" + c0.name + "' of the joined batches holds " +
                                                           std::to_string(byte_at[n]) + " bytes, more than int32 offsets can address"};
      auto ob = make_host_buffer((size_t)(total + 1) * 4 + 16);
      auto db = make_host_buffer((size_t)byte_at[n] + 16);
      int32_t* oo = (int32_t*)ob->ptr;
      oo[0] = 0;
      parallel_ranges(n, (size_t)byte_at[n] + (size_t)total * 4, [&](size_t k0, size_t k1) {
        for (size_t k = k0; k < k1; ++k) {
          const Column& c = recs[b0 + k].cols[i];
          if (!c.values || !c.length) continue;
          const int32_t* offs = (const int32_t*)c.values + c.offset;
          const int32_t first = offs[0];
          const int64_t nbytes = byte_at[k + 1] - byte_at[k];
          if (nbytes) memcpy((uint8_t*)db->ptr + byte_at[k], c.data + first, (size_t)nbytes);
          const int32_t shift = (int32_t)(byte_at[k] - first);
          int32_t* dst = oo + row_at[k];
          for (int64_t r = 1; r <= c.length; ++r) dst[r] = offs[r] + shift;
        }
      });
      o.values = (const uint8_t*)ob->ptr; o.owned.push_back(ob);
      o.data = (const uint8_t*)db->ptr; o.owned.push_back(db);
    } else {
      const size_t n = b1 - b0;
      std::vector<int64_t> row_at(n + 1, 0);
      for (size_t k = 0; k < n; ++k) row_at[k + 1] = row_at[k] + recs[b0 + k].cols[i].length;
      auto vb = make_host_buffer((size_t)total * c0.width + 16);
      parallel_ranges(n, (size_t)total * c0.width, [&](size_t k0, size_t k1) {
        for (size_t k = k0; k < k1; ++k) {
          const Column& c = recs[b0 + k].cols[i];
          if (c.length) memcpy((uint8_t*)vb->ptr + row_at[k] * c.width, c.values0(), (size_t)c.length * c.width);
        }
      });
      o.values = (const uint8_t*)vb->ptr; o.owned.push_back(vb);
    }
    cat.cols.push_back(std::move(o));
  }
  return cat;
}

void ensure_pinned_table(Context& ctx, size_t bytes) {
  ctx.pinned_tbl.reserve(bytes, bytes + bytes / 4 + 4096, "hipHostMalloc (group table)");
}

// ---- device-side concatenation of a group (general column kinds) ----------------------------------------------------
// The batches of recs[b0, b1) -- all resident in this GPU's HBM, one schema -- joined into ONE batch by the concat_*
// kernels: fixed-width values copied back to back, Utf8 offsets rebased onto one data buffer, Boolean values and validity
// bitmaps appended bit by bit.  `utf8_bytes[k][b]` = data bytes of the k-th Utf8 column of batch b (from gather_ends).
Batch concat_device_batches(Context& ctx, const std::vector<Batch>& recs, size_t b0, size_t b1,
                            const std::vector<int>& utf8_cols, const std::vector<std::vector<int64_t>>& utf8_bytes) {
  const size_t nb = b1 - b0, nc = recs[b0].cols.size();
  PhaseTimer pt("concat_device_batches");
  Batch cat;
  cat.on_device = true; cat.device_id = ctx.device;
  // ---- tables: [row_at (nb+1)] then per column [src nb] [aux nb | -] [bitoff nb | -] [byte_at nb+1 | -] [vsrc nb, vbitoff nb | -]
  struct ColPlan { size_t src = 0, aux = 0, bitoff = 0, byte_at = 0, vsrc = 0, vbitoff = 0; bool validity = false; int utf8_k = -1; };
  std::vector<ColPlan> plan(nc);
  // one pass over the batches on the pool's threads (every visit of a Batch is a cache miss at 10^4 batches): row counts
  // into a dense array, "does any batch carry nulls" per column
  std::vector<int64_t> batch_rows(nb, 0);
  {
    std::vector<std::atomic<int>> any_nulls(nc);
    for (auto& a : any_nulls) a.store(0);
    pool_ranges(nb, 2048, [&](size_t k0, size_t k1) {
      for (size_t k = k0; k < k1; ++k) {
        const Batch& rb = recs[b0 + k];
        batch_rows[k] = rb.nrows;
        for (size_t c = 0; c < nc; ++c) if (rb.cols[c].validity && rb.cols[c].null_count != 0) any_nulls[c].store(1, std::memory_order_relaxed);
      }
    });
    for (size_t c = 0; c < nc; ++c) plan[c].validity = any_nulls[c].load() != 0;
  }
  size_t words = nb + 1;
  for (size_t c = 0; c < nc; ++c) {
    const Column& c0 = recs[b0].cols[c];
    plan[c].src = words; words += nb;
    if (c0.type == T_UTF8) {
      plan[c].aux = words; words += nb;
      plan[c].byte_at = words; words += nb + 1;
      plan[c].utf8_k = (int)(std::find(utf8_cols.begin(), utf8_cols.end(), (int)c) - utf8_cols.begin());
    }
    if (c0.type == T_BOOL) { plan[c].bitoff = words; words += nb; }
    if (plan[c].validity) { plan[c].vsrc = words; words += nb; plan[c].vbitoff = words; words += nb; }
  }
  pt.mark("scan_batches");
  ensure_pinned_table(ctx, words * 8);
  u64* h = (u64*)ctx.pinned_tbl.ptr;
  int64_t total = 0;
  for (size_t k = 0; k < nb; ++k) { h[k] = (u64)total; total += batch_rows[k]; }
  h[nb] = (u64)total;
  cat.nrows = total;
  std::vector<int64_t> total_bytes(nc, 0);
  std::vector<int64_t> known_nulls(nc, 0);
  for (size_t c = 0; c < nc; ++c) {   // running byte positions first (serial, over a dense array)
    const ColPlan& pl = plan[c];
    if (recs[b0].cols[c].type != T_UTF8) continue;
    int64_t bytes = 0;
    const std::vector<int64_t>& ub = utf8_bytes[(size_t)pl.utf8_k];
    for (size_t k = 0; k < nb; ++k) { h[pl.byte_at + k] = (u64)bytes; bytes += ub[b0 + k]; }
    h[pl.byte_at + nb] = (u64)bytes; total_bytes[c] = bytes;
  }
  // the pointers: one pass over the batches (each batch's columns lie together in memory), on the pool's threads --
  // at 10^4 batches this is pointer chasing through ~10 MB of Batch / Column objects
  std::mutex nulls_m;
  pool_ranges(nb, 2048, [&](size_t k0, size_t k1) {
    std::vector<int64_t> nulls(nc, 0);
    for (size_t k = k0; k < k1; ++k) {
      const Batch& rb = recs[b0 + k];
      for (size_t c = 0; c < nc; ++c) {
        const ColPlan& pl = plan[c];
        const Column& col = rb.cols[c];
        h[pl.src + k] = (u64)(uintptr_t)(col.type == T_BOOL ? (const void*)col.values : col.values0());
        if (col.type == T_UTF8) h[pl.aux + k] = (u64)(uintptr_t)col.data;
        if (col.type == T_BOOL) h[pl.bitoff + k] = (u64)col.offset;
        if (pl.validity) {
          const bool has = col.validity && col.null_count != 0;
          h[pl.vsrc + k] = has ? (u64)(uintptr_t)col.validity : 0;
          h[pl.vbitoff + k] = (u64)col.offset;
          if (has && col.null_count > 0) nulls[c] += col.null_count;
        }
      }
    }
    std::lock_guard<std::mutex> l(nulls_m);
    for (size_t c = 0; c < nc; ++c) known_nulls[c] += nulls[c];
  });
  pt.mark("tables");
  auto d_tbl = make_device_buffer(words * 8 + 16, ctx.device);
  check_hip(hipMemcpyAsync(d_tbl->ptr, h, words * 8, hipMemcpyHostToDevice, ctx.stream), "upload concat tables");
  pt.mark("upload");
  const u64* d = (const u64*)d_tbl->ptr;
  const int grid = (int)std::min<int64_t>((int64_t)nb, (int64_t)ctx.num_cus * 16);
  for (size_t c = 0; c < nc; ++c) {
    const Column& c0 = recs[b0].cols[c];
    const ColPlan& pl = plan[c];
    Column o = empty_like(c0);
    o.length = total;
    ConcatParams cp{};
    cp.nb = (int64_t)nb; cp.row_at = (const int64_t*)d; cp.src = d + pl.src;
    if (pl.validity) {
      const size_t vbytes = (size_t)(total + 31) / 32 * 4 + 16;
      auto vb = make_device_buffer(vbytes, ctx.device);
      check_hip(hipMemsetAsync(vb->ptr, 0, vbytes, ctx.stream), "memset validity");
      ConcatParams vp = cp;
      vp.src = d + pl.vsrc; vp.bitoff = (const int64_t*)(d + pl.vbitoff); vp.dst = vb->ptr;
      check_hip(launch_concat(vp, 3, grid, ctx.stream), "launch concat_bits_kernel (validity)");
      o.validity = (const uint8_t*)vb->ptr; o.owned.push_back(vb);
      o.null_count = known_nulls[c] > 0 ? known_nulls[c] : 1;   // "may contain nulls": the filter counts what survives
    }
    if (c0.type == T_BOOL) {
      const size_t bbytes = (size_t)(total + 31) / 32 * 4 + 16;
      auto vb = make_device_buffer(bbytes, ctx.device);
      check_hip(hipMemsetAsync(vb->ptr, 0, bbytes, ctx.stream), "memset bits");
      cp.bitoff = (const int64_t*)(d + pl.bitoff); cp.dst = vb->ptr;
      check_hip(launch_concat(cp, 3, grid, ctx.stream), "launch concat_bits_kernel");
      o.values = (const uint8_t*)vb->ptr; o.owned.push_back(vb);
    } else if (c0.type == T_UTF8) {
      auto ob = make_device_buffer((size_t)(total + 1) * 4 + 16, ctx.device);
      auto db = make_device_buffer((size_t)total_bytes[c] + 16, ctx.device);
      cp.aux = d + pl.aux; cp.byte_at = (const int64_t*)(d + pl.byte_at); cp.dst = ob->ptr; cp.dst2 = db->ptr;
      if (total == 0) check_hip(hipMemsetAsync(ob->ptr, 0, 4, ctx.stream), "memset offsets");
      check_hip(launch_concat(cp, 2, grid, ctx.stream), "launch concat_utf8_kernel");
      o.values = (const uint8_t*)ob->ptr; o.owned.push_back(ob);
      o.data = (const uint8_t*)db->ptr; o.owned.push_back(db);
      o.data_bytes = total_bytes[c];
    } else {
      auto vb = make_device_buffer((size_t)total * c0.width + 16, ctx.device);
      cp.dst = vb->ptr; cp.width = c0.width;
      check_hip(launch_concat(cp, 0, grid, ctx.stream), "launch concat_fixed_kernel");
      o.values = (const uint8_t*)vb->ptr; o.owned.push_back(vb);
    }
    cat.cols.push_back(std::move(o));
  }
  check_hip(hipStreamSynchronize(ctx.stream), "hipStreamSynchronize");   // the pinned table is reused by the next chunk
  pt.mark("join_kernels");
  return cat;
}

// data bytes of every Utf8 column of every batch of a device-resident group (first / last offset read by one kernel per
// column).  Two steps: `issue` queues the kernels and the read-back, `finish` waits for them -- the one-launch path builds
// its group table in between.
struct Utf8Sizes {
  std::vector<int> cols;
  size_t nb = 0;
  BufferPtr d_tbl;
  int32_t* h_ends = nullptr;   // [cols][2 nb] in ctx.pinned_sizes
};
Utf8Sizes device_utf8_bytes_issue(Context& ctx, const GroupLite& lite, const std::vector<int>& utf8_cols) {
  Utf8Sizes z;
  z.cols = utf8_cols; z.nb = lite.rows.size();
  const size_t nb = z.nb, nu = utf8_cols.size();
  if (nu == 0) return z;
  const size_t words = (nb + 1) + nu * nb;                 // row_at, then one pointer table per column
  const size_t need = words * 8 + nu * nb * 8;
  ctx.pinned_sizes.reserve(need, need + need / 4 + 4096, "hipHostMalloc (utf8 sizes)");
  u64* h = (u64*)ctx.pinned_sizes.ptr;
  int64_t total = 0;
  for (size_t b = 0; b < nb; ++b) { h[b] = (u64)total; total += lite.rows[b]; }
  h[nb] = (u64)total;
  z.d_tbl = make_device_buffer(need + 16, ctx.device);
  z.h_ends = (int32_t*)(h + words);
  for (size_t k = 0; k < nu; ++k) {
    const size_t uc = (size_t)utf8_cols[k];
    u64* tbl = h + nb + 1 + k * nb;
    for (size_t b = 0; b < nb; ++b) tbl[b] = (u64)(uintptr_t)lite.values0[b * lite.ncols + uc];
  }
  check_hip(hipMemcpyAsync(z.d_tbl->ptr, h, words * 8, hipMemcpyHostToDevice, ctx.stream), "upload offsets tables");
  int32_t* d_ends = (int32_t*)((u64*)z.d_tbl->ptr + words);
  for (size_t k = 0; k < nu; ++k) {
    ConcatParams cp{};
    cp.nb = (int64_t)nb; cp.row_at = (const int64_t*)z.d_tbl->ptr; cp.src = (const u64*)z.d_tbl->ptr + nb + 1 + k * nb; cp.ends = d_ends + 2 * k * nb;
    check_hip(launch_concat(cp, 1, 1, ctx.stream), "launch gather_ends_kernel");
  }
  check_hip(hipMemcpyAsync(z.h_ends, d_ends, nu * nb * 8, hipMemcpyDeviceToHost, ctx.stream), "read back ends");
  return z;
}
std::vector<std::vector<int64_t>> device_utf8_bytes_finish(Context& ctx, const Utf8Sizes& z) {
  std::vector<std::vector<int64_t>> out(z.cols.size(), std::vector<int64_t>(z.nb, 0));
  if (z.cols.empty()) return out;
  check_hip(hipStreamSynchronize(ctx.stream), "hipStreamSynchronize");
  for (size_t k = 0; k < z.cols.size(); ++k) {
    const int32_t* e = z.h_ends + 2 * k * z.nb;
    for (size_t b = 0; b < z.nb; ++b) out[k][b] = (int64_t)e[2 * b + 1] - e[2 * b];
  }
  return out;
}
std::vector<std::vector<int64_t>> device_utf8_bytes(Context& ctx, const GroupLite& lite, const std::vector<int>& utf8_cols) {
  return device_utf8_bytes_finish(ctx, device_utf8_bytes_issue(ctx, lite, utf8_cols));
}

// ---- the pieces of a group call ------------------------------------------------------------------------------------------
// Chunks [cuts[k], cuts[k+1]) of a group: a cut before the batch at which the rows would pass 2^30 or the bytes of any Utf8
// column would pass `limit` (int32 offsets of the joined output; a batch over the limit on its own is a chunk of its own).
// `bytes[k][b]`: data bytes of the k-th Utf8 column of batch b.
std::vector<size_t> chunk_cuts(const std::vector<int64_t>& rows, const std::vector<std::vector<int64_t>>& bytes, int64_t limit) {
  std::vector<size_t> cuts{0};
  std::vector<int64_t> sum(bytes.size(), 0);
  int64_t at = 0;
  for (size_t b = 0; b < rows.size(); ++b) {
    bool over = at + rows[b] > (1ll << 30);
    for (size_t k = 0; k < bytes.size(); ++k) over |= sum[k] + bytes[k][b] > limit;
    if (over && b > cuts.back()) { cuts.push_back(b); std::fill(sum.begin(), sum.end(), 0); at = 0; }
    for (size_t k = 0; k < bytes.size(); ++k) sum[k] += bytes[k][b];
    at += rows[b];
  }
  cuts.push_back(rows.size());
  return cuts;
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
    Batch cat = b1 - b0 == 1 ? to_device(ctx, recs[b0]) : concat_device_batches(ctx, recs, b0, b1, utf8_cols, ubytes);
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

// ---- stage 1: eligibility -- one scan of the per-batch flags -------------------------------------------------------------
struct GroupPlan {
  bool per_batch = false;    // a batch of fewer than 2 rows, or another schema: the per-batch loop
  bool plain = false;        // fixed-width columns without nulls (wave-packed device groups: bitmaps too): the one-launch path
  bool fold = false;         // device-resident short-string Utf8 columns (`fold_utf8`): filtered straight out of the batches
  bool need_bits = false;    // validity bitmaps / Boolean columns ride along (compacted behind the main kernel)
  bool host_in = false, all_host = false;
  bool all_device = false;   // every batch in this GPU's memory
  bool resident = false;     // every batch where batch 0 is (host memory, or this GPU's)
  int64_t total_rows = 0, max_rows = 0;
  std::vector<int> fold_utf8;
};

// The facts were gathered per batch at import (GroupLite::set / set_from_arrow, on the pool's threads): here one pass over
// nb flag bytes and nb row counts, for host and device groups alike.
GroupPlan plan_group(const GroupCall& g) {
  const Context& ctx = g.ctx;
  const Batch& first = g.recs[0];
  const bool fits = (int)first.cols.size() <= MAX_OUT;
  GroupPlan pl;
  pl.host_in = !first.on_device;
  bool has_bool = false, has_utf8 = false;
  for (const Column& c : first.cols) { has_bool |= c.type == T_BOOL; has_utf8 |= c.type == T_UTF8; }
  uint8_t any = 0, all = 0xff;
  for (uint8_t f : g.lite.flags) { any |= f; all &= f; }
  if (any & (GroupLite::GL_SHORT | GroupLite::GL_SCHEMA_DIFFERS)) { pl.per_batch = true; return pl; }
  pl.all_host = (all & GroupLite::GL_ON_HOST) != 0;
  pl.all_device = (all & GroupLite::GL_ON_DEVICE) != 0;
  pl.resident = pl.host_in ? pl.all_host : pl.all_device;   // (a mixed group, or a batch on another GPU: the per-batch loop)
  // validity bitmaps and Boolean columns ride along in the one-launch path when the group is wave-packed (decided with
  // the table): their bitmaps are compacted by bit_compact_group_kernel behind the main kernel
  pl.need_bits = has_bool || (any & GroupLite::GL_NULLS);
  pl.plain = fits && !has_utf8 && (!pl.need_bits || (pl.all_device && ctx.opt_group_bits));
  // `foldable`: device-resident fixed-width or Utf8 columns -- short-string Utf8 columns can then be filtered straight out
  // of the batches by the one-launch path (their offsets and bytes per batch ride in the group table)
  const bool foldable = fits && ctx.opt_fold_utf8 && ctx.opt_group_fold && pl.all_device && !(any & GroupLite::GL_NO_UTF8_DATA) &&
                        (!pl.need_bits || ctx.opt_group_bits);
  for (int64_t r : g.lite.rows) { pl.total_rows += r; pl.max_rows = std::max(pl.max_rows, r); }
  if (!pl.plain && foldable) {
    for (size_t i = 0; i < first.cols.size(); ++i) if (first.cols[i].type == T_UTF8) pl.fold_utf8.push_back((int)i);
    pl.fold = !pl.fold_utf8.empty() && (int)pl.fold_utf8.size() <= MAX_FOLD_UTF8 && pl.total_rows < (1ll << 31) - 64;
    if (!pl.fold) pl.fold_utf8.clear();
  }
  return pl;
}

// ---- stage 2: a device group whose string columns all hold values of ONE length (the reference's sample strings, keys,
// hashes): fixed-width columns in disguise, as in filter_record -- one pass over every batch's offsets proves it, the group
// runs as a PLAIN group (value pointer of batch b = its data + its first offset) and every joined part gets back its Utf8
// columns (uniform_to_utf8).  False: a column does not qualify, or the plain group declined (e.g. a data-dependent error
// that the per-batch loop must attribute) -- the caller goes on as before.  `sizes_fit`: the fold's size check.
bool uniform_group(const GroupCall& g, const GroupPlan& pl, const std::function<bool()>& sizes_fit, GroupResult* out) {
  Context& ctx = g.ctx;
  const GroupLite& lite = g.lite;
  const size_t nb = g.nb, ncols = lite.ncols, nu = pl.fold_utf8.size();
  for (int i : pl.fold_utf8) {
    bool bitmap = false;
    for (size_t b = 0; b < nb && !bitmap; ++b) bitmap = lite.validity[b * ncols + (size_t)i] != nullptr;
    if (!uniform_utf8_ok(bitmap, pl.total_rows, 1)) return false;
  }
  // (a group whose joined strings do not fit ONE output column is cut into sub-groups first: each comes back here)
  if (!sizes_fit()) return false;
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
struct BitCol { int col; bool validity; size_t word; };   // word: index of {bitmap, bit offset} in a batch's table row
struct GroupTable {
  std::vector<BufferPtr> staged;   // host groups: every column packed and uploaded
  Batch proto;                     // batch 0 with every column that has nulls in ANY batch marked nullable
  std::vector<BitCol> bit_cols;
  std::vector<int> launch_cols;
  FilterParams p{};
  int tile_kind = 0;
  int64_t wpb = 0, ntiles = 0;     // wpb > 0: wave-granular mode
  size_t stride = 0, bits_at = 0, bytes_tbl = 0, bytes_idx = 0, bytes_cnt = 0;
};
constexpr int64_t kWaveRows[3] = {64 * 16, 64 * 8, 64 * 8};
constexpr int64_t kWavesPerTile[3] = {16, 4, 4};

// input pointers, tiling and the table (in ctx.pinned_tbl); false: the group does not fit the one-launch path after all
bool build_group_table(const GroupCall& g, const GroupPlan& pl, const Lowered& lw, GroupTable& t) {
  Context& ctx = g.ctx;
  const std::vector<Batch>& recs = g.recs;
  const GroupLite& lite = g.lite;
  const size_t nb = g.nb, ncols = recs[0].cols.size();
  const int64_t total_rows = pl.total_rows;
  ctx.stats = chq_call_stats{};
  ctx.stats.rows_in = total_rows;

  // ---- inputs: device pointers per batch and column, [batch][column] flat --------------------------------------
  // device batches: where they lie (lite.values0).  Host batches are packed column-wise into one staging block per column
  // and uploaded with one copy each: `packed` = where every batch's share of it lies in HBM
  std::vector<const uint8_t*> packed;
  if (pl.host_in) {
    packed.resize(nb * ncols);
    for (size_t i = 0; i < ncols; ++i) {
      const int64_t w = recs[0].cols[i].width;
      auto pack = make_host_buffer((size_t)(total_rows * w) + 16);   // recycled block: no page faults
      auto db = make_device_buffer((size_t)(total_rows * w) + 16, ctx.device);
      std::vector<int64_t> at(nb + 1, 0);
      for (size_t b = 0; b < nb; ++b) { at[b + 1] = at[b] + lite.rows[b] * w; packed[b * ncols + i] = (const uint8_t*)db->ptr + at[b]; }
      parallel_ranges(nb, (size_t)at[nb], [&](size_t k0, size_t k1) {
        for (size_t b = k0; b < k1; ++b) memcpy((uint8_t*)pack->ptr + at[b], lite.values0[b * ncols + i], (size_t)(lite.rows[b] * w));
      });
      check_hip(hipMemcpyAsync(db->ptr, pack->ptr, (size_t)at[nb], hipMemcpyHostToDevice, ctx.stream), "upload packed column");
      t.staged.push_back(db); t.staged.push_back(pack);
    }
    check_hip(hipStreamSynchronize(ctx.stream), "hipStreamSynchronize");
  }
  const uint8_t* const* in_ptr = pl.host_in ? packed.data() : lite.values0.data();

  // ---- tiling ------------------------------------------------------------------------------------------------
  // Wave-granular packing when the batches are near-uniform (every batch gets the wave count of the longest one and
  // at most a fifth of the waves idle); otherwise whole tiles per batch, described by a per-tile table.
  int tile_kind;
  if (lw.wide || lw.num_temps > 0) tile_kind = 2;
  else if (ctx.opt_tile_kind >= 0) tile_kind = (int)ctx.opt_tile_kind;
  else tile_kind = -1;
  {
    const int k = tile_kind < 0 ? 0 : tile_kind;
    const int64_t w = (pl.max_rows + kWaveRows[k] - 1) / kWaveRows[k];
    if (ctx.opt_group_mode != 1 && w * (int64_t)nb * kWaveRows[k] * 4 <= total_rows * 5 && w * (int64_t)nb < (1ll << 31) - 64) {
      t.wpb = w; tile_kind = k;
    } else if (ctx.opt_group_mode == 2) {
      t.wpb = w; tile_kind = k;
    }
  }
  if (tile_kind < 0) {   // the large tile unless padding every batch to a multiple of it idles more than a quarter of the lanes
    int64_t padded = 0;
    for (size_t b = 0; b < nb; ++b) padded += (lite.rows[b] + kTileRows[0] - 1) / kTileRows[0] * kTileRows[0];
    tile_kind = padded * 4 <= total_rows * 5 ? 0 : 1;
  }
  t.tile_kind = tile_kind;
  const int64_t tile_rows = kTileRows[tile_kind], wpb = t.wpb;
  if (wpb > 0) t.ntiles = (wpb * (int64_t)nb + kWavesPerTile[tile_kind] - 1) / kWavesPerTile[tile_kind];
  else for (size_t b = 0; b < nb; ++b) t.ntiles += (lite.rows[b] + tile_rows - 1) / tile_rows;
  ensure_scratch(ctx, t.ntiles);

  // ---- bitmaps (validity of any column, values of Boolean columns): wave-packed groups only --------------------------
  // `proto`: the program is lowered / pre-decoded against it (a ref that may be null must take the generic interpreter
  // even if batch 0 happens to be null-free)
  t.proto = recs[0];
  if (pl.need_bits) {
    if (wpb == 0) return false;   // ragged group: joined on the device
    // (the bitmaps' addresses and offsets come from the flat per-batch arrays: no Batch objects, as in the null-free case)
    std::vector<char> col_nulls(ncols, 0);
    for (size_t b = 0; b < nb; ++b) {
      if (!(lite.flags[b] & GroupLite::GL_NULLS)) continue;
      for (size_t i = 0; i < ncols; ++i) if (lite.validity[b * ncols + i]) col_nulls[i] = 1;
    }
    for (size_t i = 0; i < ncols; ++i) {
      Column& pc = t.proto.cols[i];
      if (col_nulls[i]) { pc.validity = (const uint8_t*)pc.values; pc.null_count = 1; }   // (never read: a marker)
      else { pc.validity = nullptr; pc.null_count = 0; }
      if (recs[0].cols[i].type == T_BOOL) t.bit_cols.push_back(BitCol{(int)i, false, 0});
      if (col_nulls[i]) t.bit_cols.push_back(BitCol{(int)i, true, 0});
    }
    if (t.bit_cols.size() > 16) return false;   // (one null counter each in the scratch header)
  }

  // column order of the launch: the stashed predicate column goes last (see filter_record)
  for (size_t i = 0; i < ncols; ++i) if (recs[0].cols[i].type != T_UTF8 && recs[0].cols[i].type != T_BOOL) t.launch_cols.push_back((int)i);
  pick_stash(t.p, ctx, lw, t.proto.cols, t.launch_cols, tile_kind);
  const size_t nrefs = lw.refs.size(), nout = t.launch_cols.size(), nu = pl.fold_utf8.size();
  t.stride = (wpb > 0 ? 1 : 2) + nrefs + nout + 2 * nu;   // per Utf8 column: the batch's offsets and bytes
  t.bits_at = pl.need_bits ? t.stride : 0;               // validity bitmap + bit offset of every program ref
  if (pl.need_bits) { t.stride += 2 * nrefs; for (BitCol& q : t.bit_cols) { q.word = t.stride; t.stride += 2; } }
  if (pl.fold && tile_kind == 2) return false;

  // ---- table (+ index of every batch's last tile in tile mode): built in pinned memory, one upload ---------------
  const size_t tbl_words = (wpb > 0 ? nb : (size_t)t.ntiles) * t.stride;
  t.bytes_tbl = tbl_words * 8; t.bytes_idx = wpb > 0 ? 0 : nb * 8; t.bytes_cnt = nb * 8;
  ensure_pinned_table(ctx, t.bytes_tbl + t.bytes_idx + t.bytes_cnt);
  u64* w = (u64*)ctx.pinned_tbl.ptr;
  int64_t* h_idx = (int64_t*)(w + tbl_words);
  int64_t tile = 0;
  for (size_t b = 0; b < nb; ++b) {
    const int64_t rows = lite.rows[b];
    const size_t at = b * ncols;
    auto value_ptrs = [&] {   // program refs, output columns, per folded Utf8 column its offsets and bytes
      for (size_t k = 0; k < nrefs; ++k) *w++ = (u64)(uintptr_t)in_ptr[at + (size_t)lw.refs[k]];
      for (size_t k = 0; k < nout; ++k) *w++ = (u64)(uintptr_t)in_ptr[at + (size_t)t.launch_cols[k]];
      for (size_t k = 0; k < nu; ++k) { *w++ = (u64)(uintptr_t)in_ptr[at + (size_t)pl.fold_utf8[k]]; *w++ = (u64)(uintptr_t)lite.data[at + (size_t)pl.fold_utf8[k]]; }
    };
    if (wpb > 0) {
      *w++ = (u64)rows;
      value_ptrs();
      if (pl.need_bits) {
        for (size_t k = 0; k < nrefs; ++k) *w++ = (u64)(uintptr_t)lite.validity[at + (size_t)lw.refs[k]];
        for (size_t k = 0; k < nrefs; ++k) *w++ = (u64)lite.offset[at + (size_t)lw.refs[k]];
        for (const BitCol& q : t.bit_cols) {
          *w++ = (u64)(uintptr_t)(q.validity ? lite.validity[at + (size_t)q.col] : lite.values0[at + (size_t)q.col]);   // (a Boolean column's values0 is its bitmap)
          *w++ = (u64)lite.offset[at + (size_t)q.col];
        }
      }
      continue;
    }
    for (int64_t r0 = 0; r0 < rows; r0 += tile_rows, ++tile) {
      *w++ = (u64)r0; *w++ = (u64)rows;
      value_ptrs();
    }
    h_idx[b] = tile - 1;   // rows >= 2: every batch owns at least one tile
  }
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
  const int64_t total_rows = pl.total_rows, ntiles = t.ntiles, wpb = t.wpb;
  const int tile_kind = t.tile_kind;
  FilterParams& p = t.p;
  PhaseTimer pt("filter_records (launch)");
  u64* h_cnt = (u64*)((uint8_t*)ctx.pinned_tbl.ptr + t.bytes_tbl + t.bytes_idx);
  auto d_tbl = make_device_buffer(t.bytes_tbl + t.bytes_idx + t.bytes_cnt + 16, ctx.device);
  check_hip(hipMemcpyAsync(d_tbl->ptr, ctx.pinned_tbl.ptr, t.bytes_tbl + t.bytes_idx, hipMemcpyHostToDevice, ctx.stream), "upload group table");
  u64* d_cnt = (u64*)((uint8_t*)d_tbl->ptr + t.bytes_tbl + t.bytes_idx);
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
    p.sel_mask = (u64*)g_sel->ptr; p.grp_base = (u64*)g_base->ptr; p.group_bits_at = (int32_t)t.bits_at; p.pb.group_bits_at = (int32_t)t.bits_at;
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
  p.group = (const u64*)d_tbl->ptr; p.group_stride = (int64_t)t.stride;
  p.group_wpb = (int32_t)wpb; p.group_nb = (int32_t)nb; p.group_batch_end = d_cnt;
  p.tile_begin = 0; p.tile_end = ntiles;
  clear_scratch(ctx, ntiles);
  kernel_span_begin(ctx);
  check_hip(launch_filter(p, tile_kind, true, (int)std::min<int64_t>(ntiles, grid_cap(ctx, tile_kind)), ctx.stream), "launch filter_fused_kernel (group)");
  kernel_span_end(ctx);
  ctx.stats.launches = 1; ctx.stats.tiles = ntiles;
  if (wpb == 0) {   // tile mode: the inclusive prefix at every batch's last tile
    GatherStatusParams gp{};
    gp.status = dev_status(ctx); gp.idx = (const int64_t*)((const uint8_t*)d_tbl->ptr + t.bytes_tbl);
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
    bp.sel_mask = (const u64*)g_sel->ptr; bp.grp_base = (const u64*)g_base->ptr; bp.table = (const u64*)d_tbl->ptr; bp.stride = (int64_t)t.stride;
    bp.word_ptr = (int32_t)t.bit_cols[q].word; bp.word_off = (int32_t)t.bit_cols[q].word + 1; bp.wpb = (int32_t)wpb; bp.nb = (int32_t)nb;
    bp.rows_per_wave = (int32_t)kWaveRows[tile_kind]; bp.out_bits = (uint32_t*)bit_out[q]->ptr;
    bp.zero_count = t.bit_cols[q].validity ? &ds->counters[q] : nullptr;
    check_hip(launch_bit_compact_group(bp, (int)std::min<int64_t>((wpb * (int64_t)nb + 3) / 4, (int64_t)ctx.num_cus * 8), ctx.stream), "launch bit_compact_group_kernel");
    ++ctx.stats.launches;
  }
  check_hip(hipMemcpyAsync(h_cnt, d_cnt, t.bytes_cnt, hipMemcpyDeviceToHost, ctx.stream), "read back batch prefixes");
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
  bool groups_of_two = cuts.size() > 2;
  for (size_t k = 0; k + 1 < cuts.size(); ++k) groups_of_two = groups_of_two && cuts[k + 1] - cuts[k] >= 2;
  if (!groups_of_two) return false;
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
  // the batches' string sizes are read back from the device: queued here, awaited only after the predicate has been typed
  // and the group table built (`sizes_fit` below)
  Utf8Sizes sizes_in_flight;
  if (pl.fold) sizes_in_flight = device_utf8_bytes_issue(ctx, g.lite, pl.fold_utf8);
  std::vector<std::vector<int64_t>> fold_bytes;   // bytes of every folded Utf8 column per batch
  std::vector<int64_t> fold_cap;                  // and in all
  bool sizes_done = false, sizes_ok = false;
  auto sizes_fit = [&]() -> bool {   // false: long strings, or more than one output column can address
    if (sizes_done) return sizes_ok;
    sizes_done = true;
    fold_bytes = device_utf8_bytes_finish(ctx, sizes_in_flight);
    bool ok = true;
    for (const auto& per_batch : fold_bytes) {
      int64_t cap = 0;
      for (int64_t v : per_batch) cap += v;
      fold_cap.push_back(cap);
      // short strings that fit ONE output column (int32 offsets: 2 x group_chunk_bytes = 2 GiB unless a test lowers the option)
      ok &= cap <= pl.total_rows * 24 && cap < 2 * ctx.opt_group_chunk_bytes - 64;
    }
    sizes_ok = ok;
    return ok;
  };
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
    if (!sizes_in_flight.cols.empty()) check_hip(hipStreamSynchronize(ctx.stream), "hipStreamSynchronize");   // (the size gather reads back into pinned memory the next call reuses)
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
    if (uniform_group(g, pl, sizes_fit, &r)) return r;
  }
  // the predicate itself must not read a string column, and the wide / temporaries instantiation has no Utf8 form
  if (pl.fold && (reads_utf8 || lw.wide || lw.num_temps > 0)) return other_path();

  GroupTable t;
  if (!build_group_table(g, pl, lw, t)) return other_path();
  pt.mark("table");
  if (pl.fold && !sizes_fit()) {
    bool short_strings = !coalesce;
    for (int64_t cap : fold_cap) short_strings = short_strings && cap <= pl.total_rows * 24;
    GroupResult r;
    if (short_strings && split_short_strings(g, fold_bytes, &r)) return r;
    return other_path();   // (long strings / too many bytes for one column: joined on the device)
  }
  pt.mark("utf8_sizes");
  GroupResult r;
  r.parts.emplace_back();
  if (!launch_group(g, pl, lw, t, fold_cap, r.parts[0])) return g.per_batch_loop();
  return r;
}
}  // namespace

// sort.hpp
Batch join_group(Context& ctx, const std::vector<Batch>& recs) {
  std::vector<Batch> dev(recs.size());
  for (size_t b = 0; b < recs.size(); ++b) dev[b] = to_device(ctx, recs[b]);
  if (dev.size() == 1) return std::move(dev[0]);
  std::vector<int> utf8_cols;
  for (size_t c = 0; c < dev[0].cols.size(); ++c) if (dev[0].cols[c].type == T_UTF8) utf8_cols.push_back((int)c);
  GroupLite lite;
  lite.resize(dev.size(), dev[0].cols.size());
  for (size_t b = 0; b < dev.size(); ++b) lite.set(b, dev[b], dev[0], ctx.device);
  const auto bytes = device_utf8_bytes(ctx, lite, utf8_cols);
  for (size_t k = 0; k < utf8_cols.size(); ++k) {
    int64_t total = 0;
    for (int64_t x : bytes[k]) total += x;
    if (total > INT32_MAX)
      throw ChqError{CHQ_ERR_ARROW_INVALID_ARGUMENT, "Utf8 column '" + dev[0].cols[(size_t)utf8_cols[k]].name + "' of the joined group holds " +
                                                     std::to_string(total) + " bytes, more than int32 offsets can address"};
  }
  return concat_device_batches(ctx, dev, 0, dev.size(), utf8_cols, bytes);
}

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

// ---- GroupLite: the per-batch facts of a group (engine.hpp) ----------------------------------------------------------------
// `set` reads an imported batch, `set_from_arrow` the Arrow structs of a device batch (the checks of import_batch, but no
// Batch object).  Both run per batch on the pool's threads and allocate nothing.  They must agree on: the residency bits,
// GL_SHORT below 2 rows, GL_SCHEMA_DIFFERS for anything the group paths cannot take (the full import then decides and
// reports), and per column what `put_column` stores -- values0 with the slice offset applied (Boolean: the bitmap itself),
// the Utf8 bytes, the bit offset, and the validity bitmap only where it may clear a bit.
// One column (type and width of `kind`) of one batch into slot `at`; returns the GL_* bits it contributes.
static uint8_t put_column(GroupLite& g, size_t at, const Column& kind, bool on_host, const uint8_t* bitmap, int64_t null_count,
                          int64_t length, const uint8_t* values, const uint8_t* bytes, int64_t off) {
  uint8_t f = 0;
  // nulls: a device batch with a bitmap and null_count != 0 counts as having them; a host batch that has not counted
  // (null_count < 0) is counted here, and a bitmap with every bit set is no bitmap
  bool nulls = bitmap && null_count != 0;
  if (nulls && on_host && null_count < 0) nulls = count_nulls_host(bitmap, off, length) != 0;
  if (nulls) { f |= GroupLite::GL_NULLS; g.validity[at] = bitmap; }
  if (kind.type == T_UTF8 && !bytes) f |= GroupLite::GL_NO_UTF8_DATA;
  g.values0[at] = !values || kind.type == T_BOOL ? values : values + (int64_t)(kind.type == T_UTF8 ? 4 : kind.width) * off;
  g.data[at] = bytes;
  g.offset[at] = off;
  return f;
}

void GroupLite::set(size_t b, const Batch& r, const Batch& first, int device) {
  rows[b] = r.nrows;
  uint8_t f = 0;
  if (!r.on_device) f |= GL_ON_HOST;
  if (r.on_device && r.device_id == device) f |= GL_ON_DEVICE;
  if (r.nrows < 2) f |= GL_SHORT;
  if (r.cols.size() != ncols) { flags[b] = (uint8_t)(f | GL_SCHEMA_DIFFERS); return; }
  for (size_t i = 0; i < ncols; ++i) {
    const Column& c = r.cols[i];
    const Column& c0 = first.cols[i];
    if (c.type != c0.type || c.width != c0.width || c.format != c0.format) f |= GL_SCHEMA_DIFFERS;
    f |= put_column(*this, b * ncols + i, c, !r.on_device, c.validity, c.null_count, c.length, c.values, c.data, c.offset);
  }
  flags[b] = f;
}

void GroupLite::set_from_arrow(size_t b, const ArrowDeviceArray* rec, const ArrowSchema* schema, const Batch& first, int device) {
  const ArrowArray& a = rec->array;
  if (a.offset != 0 || a.n_children != schema->n_children || (size_t)a.n_children != ncols || rec->device_type != ARROW_DEVICE_ROCM || rec->sync_event) {
    flags[b] = GL_SCHEMA_DIFFERS;   // (anything unusual: the full import decides -- and reports)
    return;
  }
  rows[b] = a.length;
  uint8_t f = 0;
  if ((int)rec->device_id == device) f |= GL_ON_DEVICE;
  if (a.length < 2) f |= GL_SHORT;
  for (size_t i = 0; i < ncols; ++i) {
    const ArrowArray* ca = a.children[i];
    if (!ca || ca->length < a.length || ca->offset < 0 || ca->n_buffers < 2 || !ca->buffers || !ca->buffers[1] ||
        (ca->null_count > 0 && !ca->buffers[0])) { f |= GL_SCHEMA_DIFFERS; continue; }
    const Column& c0 = first.cols[i];
    const uint8_t* bytes = c0.type == T_UTF8 && ca->n_buffers > 2 ? (const uint8_t*)ca->buffers[2] : nullptr;
    f |= put_column(*this, b * ncols + i, c0, false, (const uint8_t*)ca->buffers[0], ca->null_count, a.length, (const uint8_t*)ca->buffers[1], bytes, ca->offset);
  }
  flags[b] = f;
}

GroupLite GroupLite::slice(size_t b0, size_t b1) const {
  GroupLite s;
  s.ncols = ncols;
  s.rows.assign(rows.begin() + b0, rows.begin() + b1);
  s.flags.assign(flags.begin() + b0, flags.begin() + b1);
  s.values0.assign(values0.begin() + b0 * ncols, values0.begin() + b1 * ncols);
  s.data.assign(data.begin() + b0 * ncols, data.begin() + b1 * ncols);
  s.validity.assign(validity.begin() + b0 * ncols, validity.begin() + b1 * ncols);
  s.offset.assign(offset.begin() + b0 * ncols, offset.begin() + b1 * ncols);
  return s;
}

}  // namespace chq
