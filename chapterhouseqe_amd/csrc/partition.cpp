// partition.cpp -- hash partitioning on the device (chq_partition_records).
//
// Every row gets a partition id, a pinned function of the bits of its key values (include/chq.h), computed from the key
// columns in place.  The ids are then treated like the digit of ONE radix pass of the sort: per-tile counts, a scan per
// partition, and a scatter of the row ids, which is stable.  Only the ids (1 byte) and the permutation (4 bytes) move per
// row; the rows themselves move once, when gather_column applies the permutation to every column.  Two read-backs: the rows
// per partition (they are the `ends` of the outputs) and one block of null counts at the end.  DESIGN.md section 3.9.
//
// Out of scope: expressions as keys, range partitioning, more than 256 partitions per call.
#include <algorithm>
#include <cstring>
#include <string>

#include "partition.hpp"

namespace chq {
namespace {

constexpr int64_t kMaxPartitionRows = (int64_t)1 << 32;   // row ids are u32

}  // namespace

JoinedGroup partition_records(Context& ctx, std::vector<Batch>& in, const chq_table_aliases* aliases, const std::vector<const Expr*>& keys,
                              int n_partitions) {
  if (in.empty()) throw ChqError{CHQ_ERR_ARROW_INVALID_ARGUMENT, "at least one record batch is needed"};
  if (keys.empty()) throw ChqError{CHQ_ERR_ARROW_INVALID_ARGUMENT, "a partitioning needs at least one key column"};
  if (n_partitions < 1 || n_partitions > kPartMaxPartitions)
    throw ChqError{CHQ_ERR_ARROW_INVALID_ARGUMENT, "n_partitions must be in [1, " + std::to_string(kPartMaxPartitions) + "] (" +
                                                   std::to_string(n_partitions) + " given)"};
  int64_t rows = 0;
  for (const Batch& b : in) rows += b.nrows;
  if (rows >= kMaxPartitionRows)
    throw ChqError{CHQ_ERR_NOT_SUPPORTED, "a partitioning takes fewer than 2^32 rows per call (" + std::to_string(rows) + " given)"};
  // ---- 1. keys resolve and type-check against the schema before any data moves
  const auto pcols = plan_columns(in[0], aliases);
  std::vector<int> cols;
  for (const Expr* e : keys) {
    if (!e) throw ChqError{CHQ_ERR_INVALID_HANDLE, "null partition key"};
    const int c = resolve_key(*e, pcols, rows, "a partition key");
    const Column& col = in[0].cols[(size_t)c];
    if (!sortable(col))
      throw ChqError{CHQ_ERR_NOT_SUPPORTED, "partition key '" + col.name + "' has Arrow type '" + col.format + "', which has no order in this build"};
    cols.push_back(c);
  }

  // ---- 2. one device batch
  ctx.stats = chq_call_stats{};
  const Batch rec = join_group(ctx, in);
  const int64_t n = rec.nrows, ntiles = (n + kPartTile - 1) / kPartTile;
  const size_t P = (size_t)n_partitions;
  ctx.stats.rows_in = n; ctx.stats.rows_out = n; ctx.stats.tiles = ntiles;
  kernel_span_begin(ctx);
  Traffic t;
  JoinedGroup out;
  out.ends.assign(P, n);   // (one partition: every row, in input order)
  BufferPtr perm_buf;
  if (n > 0 && P > 1) {
    // ---- 3. hash (+ count) -> scan -> scatter
    BufferPtr ids = make_device_buffer((size_t)n + 16, ctx.device);
    BufferPtr tiles = make_device_buffer(P * (size_t)ntiles * 4 + 16, ctx.device);
    BufferPtr totals = make_device_buffer(P * 4 + 16, ctx.device);
    BufferPtr carry = cols.size() > (size_t)kPartMaxKeys ? make_device_buffer((size_t)n * 8 + 16, ctx.device) : nullptr;
    perm_buf = make_device_buffer((size_t)n * 4 + 16, ctx.device);
    check_hip(hipMemsetAsync(totals->ptr, 0, P * 4, ctx.stream), "hipMemsetAsync");
    PartHashParams hp{};
    hp.n = n; hp.ntiles = ntiles; hp.n_partitions = (uint32_t)P; hp.carry = carry ? (uint64_t*)carry->ptr : nullptr;
    hp.ids = (uint8_t*)ids->ptr; hp.tile_counts = (uint32_t*)tiles->ptr; hp.totals = (uint32_t*)totals->ptr;
    for (size_t k0 = 0; k0 < cols.size(); k0 += (size_t)hp.n_keys) {
      hp.n_keys = (int32_t)std::min<size_t>(kPartMaxKeys, cols.size() - k0);
      hp.first = k0 == 0 ? 1 : 0;
      hp.last = k0 + (size_t)hp.n_keys == cols.size() ? 1 : 0;
      for (int q = 0; q < hp.n_keys; ++q) {
        const Column& c = rec.cols[(size_t)cols[k0 + (size_t)q]];
        PartKey& key = hp.keys[q];
        key = PartKey{};
        key.validity = c.live_validity();
        key.bit_offset = c.offset;
        key.values = (const uint8_t*)c.values0();
        key.data = c.data;
        key.kind = c.type == T_BOOL ? PK_BOOL : c.type == T_UTF8 ? PK_UTF8 : PK_FIXED;
        key.width = c.width;
        t.read += n * (c.type == T_UTF8 ? 8 + (c.length ? std::max<int64_t>(c.data_bytes, 0) / c.length : 0) : std::max(1, c.width));
      }
      check_hip(launch_part_hash(hp, ctx.stream), "launch part_hash_kernel");
      ++ctx.stats.launches;
      t.read += hp.first ? 0 : n * 8;
      t.written += hp.last ? n + (int64_t)P * ntiles * 4 : n * 8;
    }
    PartScatterParams sp{};
    sp.n = n; sp.ntiles = ntiles; sp.ids = hp.ids; sp.tile_counts = hp.tile_counts; sp.totals = hp.totals; sp.n_partitions = (uint32_t)P;
    sp.perm = (uint32_t*)perm_buf->ptr;
    check_hip(launch_part_scatter(sp, ctx.stream), "launch part_scan/scatter_kernel");
    ctx.stats.launches += 2;
    t.read += (int64_t)P * ntiles * 4 * 2 + n; t.written += (int64_t)P * ntiles * 4 + n * 4;
    // ---- 4. the rows per partition are the ends of the outputs
    std::vector<uint32_t> h(P);
    check_hip(hipMemcpyAsync(h.data(), totals->ptr, P * 4, hipMemcpyDeviceToHost, ctx.stream), "read back the rows per partition");
    check_hip(hipStreamSynchronize(ctx.stream), "hipStreamSynchronize");
    int64_t end = 0;
    for (size_t p = 0; p < P; ++p) { end += (int64_t)h[p]; out.ends[p] = end; }
    if (end != n) throw ChqError{CHQ_ERR_DEVICE, "internal error: the partitions hold " + std::to_string(end) + " of " + std::to_string(n) + " rows"};
  }

  // ---- 5. every column through the permutation
  const uint32_t* perm = perm_buf ? (const uint32_t*)perm_buf->ptr : nullptr;
  const size_t nc = rec.cols.size();
  BufferPtr ones = make_device_buffer(nc * 8 + 16, ctx.device);
  check_hip(hipMemsetAsync(ones->ptr, 0, nc * 8 + 16, ctx.stream), "hipMemsetAsync");
  out.joined.nrows = n; out.joined.on_device = true; out.joined.device_id = ctx.device;
  for (size_t ci = 0; ci < nc; ++ci) out.joined.cols.push_back(gather_column(ctx, rec.cols[ci], perm, n, (uint64_t*)ones->ptr + ci, t));
  fill_null_counts(out.joined.cols, n, finish_call(ctx, ones->ptr, nc, t));
  return out;
}

}  // namespace chq
