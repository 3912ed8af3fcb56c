// group_concat.cpp -- the batches of a group joined into ONE batch, on the host or by the concat_* kernels, and the size gather
// in front of the device join.  The group filter's concat paths (group.cpp) and, through join_group (sort.hpp), ORDER BY,
// GROUP BY, JOIN, the window functions and the hash partitioning stand on these.
#include "engine_internal.hpp"

#include <atomic>
#include <cstring>
#include <mutex>

namespace chq {
namespace {
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
}  // namespace

// ---- host-side concatenation of a group (general column kinds) -----------------------------------------------
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

// ---- device-side concatenation of a group (general column kinds) ----------------------------------------------------
// The batches of recs[b0, b1) -- all resident in this GPU's HBM, one schema -- joined into ONE batch by the concat_*
// kernels: fixed-width values copied back to back, Utf8 offsets rebased onto one data buffer, Boolean values and validity
// bitmaps appended bit by bit.  `utf8_bytes[k][b]` = data bytes of the k-th Utf8 column of batch b (from gather_ends).
// The tables the kernels read are laid out by layout_concat (group_plan.hpp).
Batch concat_device_batches(Context& ctx, const std::vector<Batch>& recs, size_t b0, size_t b1,
                            const std::vector<std::vector<int64_t>>& utf8_bytes) {
  const size_t nb = b1 - b0, nc = recs[b0].cols.size();
  PhaseTimer pt("concat_device_batches");
  Batch cat;
  cat.on_device = true; cat.device_id = ctx.device;
  // one pass over the batches on the pool's threads (every visit of a Batch is a cache miss at 10^4 batches): row counts
  // into a dense array, "does any batch carry nulls" per column
  std::vector<int64_t> batch_rows(nb, 0);
  std::vector<char> has_nulls(nc, 0);
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
    for (size_t c = 0; c < nc; ++c) has_nulls[c] = any_nulls[c].load() != 0;
  }
  std::vector<GroupCol> schema;
  for (const Column& c : recs[b0].cols) schema.push_back(GroupCol{c.type, c.width});
  const ConcatLayout lay = layout_concat(schema, nb, has_nulls);
  const std::vector<ConcatCol>& plan = lay.cols;
  const size_t words = lay.words;
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
    const ConcatCol& pl = plan[c];
    if (pl.utf8_k < 0) continue;
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
        const ConcatCol& pl = plan[c];
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
    const ConcatCol& pl = plan[c];
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
  return concat_device_batches(ctx, dev, 0, dev.size(), bytes);
}

}  // namespace chq
