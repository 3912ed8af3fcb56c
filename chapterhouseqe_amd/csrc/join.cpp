// join.cpp -- JOIN on the device (chq_join_records, chq_join_records_kind): a sort-merge equi-join; INNER, LEFT, RIGHT, FULL,
// LEFT_SEMI and LEFT_ANTI.
//
// The key columns of both sides are concatenated into one key batch, RIGHT rows first, and ordered by the stable sort of
// sort.cpp; GROUP BY's run finder (aggregate.hpp: find_runs) then numbers the runs of equal keys.  Because the sort is stable and the
// right rows come first, a run lies in the sorted positions as [its right rows in input order][its left rows in input order].
// The kernels of join.hip find where the left rows of every run begin, count the matches of every left row, scan the counts
// over the left rows in input order and expand them into two row-id lists, which gather_column turns into the output columns.
// Three read-backs besides the sort's: the number of runs, the number of output rows (it sizes every output), and one block
// of null counts at the end.
//
// The other kinds change the count rule and let a row-id list say "no row" (kJoinNoRow), which the padded gathers turn into a
// null: LEFT counts max(c, 1) and an unmatched left row writes "no row" for its right row; SEMI counts c > 0 and ANTI c == 0
// and neither has a right list; FULL is LEFT followed by a tail of the right rows in runs with a null key or without left
// rows, found in one pass over the sorted positions and placed by the same scan (its length comes back with the row count, in
// the same wait).  RIGHT is LEFT with the sides exchanged and the columns put back.  A side without rows skips the kernels:
// the lists are the identity (no list) and "no row" everywhere (a memset).  DESIGN.md section 3.8.
//
// Out of scope: CROSS joins, non-equality conditions, expressions as keys, coercion between key types, the SQL grammar of
// the kinds other than INNER.  A call is single-instance: a partitioned or multi-instance join partitions both sides by the
// keys first (partition.cpp) and makes one call per partition.
#include <algorithm>
#include <cstring>
#include <string>

#include "join.hpp"

namespace chq {
namespace {

constexpr int64_t kMaxJoinRows = (int64_t)1 << 32;   // sorted positions, row ids and output rows are u32

int resolve_join_key(const Expr* e, const char* side, const std::vector<PlanColumn>& pcols, int64_t rows) {
  if (!e) throw ChqError{CHQ_ERR_INVALID_HANDLE, std::string("null ") + side + " join key"};
  return resolve_key(*e, pcols, rows, "a join key");
}

// The key columns of one side as batches of their own, appended to `out`: zero-copy views under the names both sides share,
// cut into slices of rows.  The concat kernels give every batch ONE workgroup: a side handed over in one piece would be
// copied by a single workgroup, in slices the copy spreads over the device.
constexpr int64_t kKeySliceRows = 16384;   // at least this many rows per slice ...
constexpr int64_t kKeySlices = 2048;       // ... and at most about this many slices per side

void key_views(const Batch& side, const std::vector<int>& cols, const std::vector<std::string>& names, std::vector<Batch>& out) {
  const int64_t step = std::max(kKeySliceRows, (side.nrows + kKeySlices - 1) / kKeySlices);
  for (int64_t r0 = 0; r0 < side.nrows; r0 += step) {
    Batch kb;
    kb.nrows = std::min(step, side.nrows - r0); kb.on_device = side.on_device; kb.device_id = side.device_id;
    for (size_t k = 0; k < cols.size(); ++k) {
      Column c = side.cols[(size_t)cols[k]];
      c.name = names[k];
      c.nullable = true;
      if (kb.nrows != side.nrows) {   // a slice: what the column knew about all of its rows no longer holds
        c.offset += r0; c.length = kb.nrows;
        if (c.validity && c.null_count != 0) c.null_count = -1;
        c.data_bytes = -1;
      }
      kb.cols.push_back(std::move(c));
    }
    out.push_back(std::move(kb));
  }
}

// the join of kind INNER, LEFT, FULL, LEFT_SEMI or LEFT_ANTI over keys already resolved to columns
Batch join_resolved(Context& ctx, std::vector<Batch>& left, std::vector<Batch>& right, const std::vector<int>& cols_l,
                    const std::vector<int>& cols_r, const std::vector<std::string>& key_names, int kind) {
  const bool pad_right = kind == CHQ_JOIN_LEFT || kind == CHQ_JOIN_FULL, pad_left = kind == CHQ_JOIN_FULL;
  const bool left_only = kind == CHQ_JOIN_LEFT_SEMI || kind == CHQ_JOIN_LEFT_ANTI;
  const size_t n_keys = cols_l.size();
  // ---- 2. one device batch per side
  ctx.stats = chq_call_stats{};
  const Batch L = join_group(ctx, left);
  const Batch R = join_group(ctx, right);
  const int64_t nL = L.nrows, nR = R.nrows, n = nL + nR, ntiles = (n + kJoinTile - 1) / kJoinTile;
  ctx.stats.rows_in = n; ctx.stats.tiles = ntiles;
  kernel_span_begin(ctx);
  Traffic t;
  int64_t M = 0;
  BufferPtr lidx, ridx;
  auto no_rows = [&](int64_t m) {   // a list of m times "no row"
    BufferPtr b = make_device_buffer((size_t)m * 4 + 16, ctx.device);
    check_hip(hipMemsetAsync(b->ptr, 0xFF, (size_t)m * 4, ctx.stream), "hipMemsetAsync");
    t.written += m * 4;
    return b;
  };
  if (nR == 0 && nL > 0 && (pad_right || kind == CHQ_JOIN_LEFT_ANTI)) {   // every left row is unmatched: the identity list
    M = nL;
    if (pad_right) ridx = no_rows(M);
  } else if (nL == 0 && nR > 0 && pad_left) {                             // every right row is unmatched
    M = nR;
    lidx = no_rows(M);
  } else if (nL > 0 && nR > 0) {
    // ---- 3. the keys of both sides in one batch, right rows first; 4. their stable order
    std::vector<Batch> key_batches;
    key_views(R, cols_r, key_names, key_batches);
    key_views(L, cols_l, key_names, key_batches);
    const Batch K = join_group(ctx, key_batches);
    std::vector<int> key_cols(n_keys);
    for (size_t k = 0; k < n_keys; ++k) key_cols[k] = (int)k;
    const std::vector<SortKeyArg> sort_keys(n_keys, SortKeyArg{nullptr, false, false});
    const BufferPtr perm_buf = sort_permutation(ctx, K, key_cols, sort_keys, t);
    const uint32_t* perm = perm_buf ? (const uint32_t*)perm_buf->ptr : nullptr;

    // ---- 5. the runs of equal keys: ids, starts
    const Runs runs = find_runs(ctx, K, perm, key_cols, t);
    const int64_t G = runs.G;
    const uint32_t* const gids = (const uint32_t*)runs.gids->ptr;
    const uint32_t* const starts = (const uint32_t*)runs.starts->ptr;

    // ---- 6. split -> count -> scan (read back M) -> expand
    BufferPtr split = make_device_buffer((size_t)G * 4 + 16, ctx.device);
    JoinSplitParams sp{};
    sp.perm = perm; sp.n = n; sp.n_right = nR; sp.gids = gids; sp.starts = starts; sp.split = (uint32_t*)split->ptr;
    for (size_t k0 = 0; k0 < key_cols.size(); k0 += (size_t)sp.n_keys) {
      sp.n_keys = (int32_t)std::min<size_t>(kAggMaxKeys, key_cols.size() - k0);
      sp.nulls_only = k0 ? 1 : 0;
      bool any_nulls = false;
      for (int q = 0; q < sp.n_keys; ++q) {
        const Column& c = K.cols[k0 + (size_t)q];
        sp.validity[q] = c.live_validity();
        sp.bit_offset[q] = c.offset;
        any_nulls |= sp.validity[q] != nullptr;
      }
      if (k0 && !any_nulls) continue;   // (a later launch only applies the null rule)
      check_hip(launch_join_split(sp, ctx.stream), "launch join_split_kernel");
      ++ctx.stats.launches;
      t.read += n * 8 + G * 4; t.written += G * 4;
    }
    const int64_t ltiles = (nL + kJoinTile - 1) / kJoinTile;
    BufferPtr cnt = make_device_buffer((size_t)nL * 4 + 16, ctx.device);
    BufferPtr first = make_device_buffer((size_t)nL * 4 + 16, ctx.device);
    BufferPtr off = make_device_buffer((size_t)nL * 4 + 16, ctx.device);
    BufferPtr sums = make_device_buffer((size_t)(ltiles + 1) * 8 + 16, ctx.device);
    JoinCountParams cp{};
    cp.perm = perm; cp.n = n; cp.n_right = nR; cp.gids = gids; cp.starts = starts; cp.split = sp.split;
    cp.cnt = (uint32_t*)cnt->ptr; cp.first = (uint32_t*)first->ptr;
    if (kind == CHQ_JOIN_INNER) {
      check_hip(launch_join_count(cp, ctx.stream), "launch join_count_kernel");
    } else {
      JoinCountKindParams kp{};
      kp.base = cp;
      kp.rule = pad_right ? JOIN_COUNT_PADDED : kind == CHQ_JOIN_LEFT_SEMI ? JOIN_COUNT_SEMI : JOIN_COUNT_ANTI;
      check_hip(launch_join_count_kind(kp, ctx.stream), "launch join_count_kind_kernel");
    }
    ++ctx.stats.launches;
    t.read += n * 8 + nL * 8; t.written += left_only ? nL * 4 : nL * 8;
    OffsetsScanParams scp{};
    scp.len = cp.cnt; scp.n = nL; scp.ntiles = ltiles; scp.tile_sums = (uint64_t*)sums->ptr; scp.out = (uint32_t*)off->ptr;
    check_hip(launch_offsets_scan(scp, ctx.stream), "launch the offsets scan of the left rows");
    ctx.stats.launches += 3;
    t.read += nL * 8 + ltiles * 24; t.written += nL * 4 + ltiles * 16;
    // FULL: the right rows nobody matched, flagged in right input order and scanned like the counts
    const int64_t rtiles = (nR + kJoinTile - 1) / kJoinTile;
    BufferPtr flag, roff, rsums;
    JoinTailParams tp{};
    if (pad_left) {
      flag = make_device_buffer((size_t)nR * 4 + 16, ctx.device);
      roff = make_device_buffer((size_t)nR * 4 + 16, ctx.device);
      rsums = make_device_buffer((size_t)(rtiles + 1) * 8 + 16, ctx.device);
      tp.perm = perm; tp.n = n; tp.n_right = nR; tp.gids = gids; tp.starts = starts; tp.split = sp.split;
      tp.flag = (uint32_t*)flag->ptr; tp.off = (const uint32_t*)roff->ptr;
      check_hip(launch_join_tail_flag(tp, ctx.stream), "launch join_tail_flag_kernel");
      ++ctx.stats.launches;
      t.read += n * 8 + nR * 12; t.written += nR * 4;
      OffsetsScanParams rsp{};
      rsp.len = tp.flag; rsp.n = nR; rsp.ntiles = rtiles; rsp.tile_sums = (uint64_t*)rsums->ptr; rsp.out = (uint32_t*)roff->ptr;
      check_hip(launch_offsets_scan(rsp, ctx.stream), "launch the offsets scan of the right rows");
      ctx.stats.launches += 3;
      t.read += nR * 8 + rtiles * 24; t.written += nR * 4 + rtiles * 16;
    }
    uint64_t m64 = 0, u64 = 0;
    check_hip(hipMemcpyAsync(&m64, scp.tile_sums + ltiles, 8, hipMemcpyDeviceToHost, ctx.stream), "read back the output row count");
    if (pad_left)
      check_hip(hipMemcpyAsync(&u64, (uint64_t*)rsums->ptr + rtiles, 8, hipMemcpyDeviceToHost, ctx.stream), "read back the unmatched right rows");
    check_hip(hipStreamSynchronize(ctx.stream), "hipStreamSynchronize");
    if (u64 > (uint64_t)nR) throw ChqError{CHQ_ERR_DEVICE, "internal error: " + std::to_string(u64) + " unmatched right rows of " + std::to_string(nR)};
    if (m64 + u64 >= (uint64_t)kMaxJoinRows)
      throw ChqError{CHQ_ERR_NOT_SUPPORTED, "the join would produce " + std::to_string(m64 + u64) + " rows; a call returns fewer than 2^32"};
    const int64_t m_left = (int64_t)m64;
    M = m_left + (int64_t)u64;
    if (M > 0) {
      lidx = make_device_buffer((size_t)M * 4 + 16, ctx.device);
      if (!left_only) ridx = make_device_buffer((size_t)M * 4 + 16, ctx.device);
      JoinExpandParams ep{};
      ep.perm = perm; ep.off = scp.out; ep.first = cp.first; ep.n_left = nL; ep.m = m_left;
      ep.lidx = (uint32_t*)lidx->ptr; ep.ridx = ridx ? (uint32_t*)ridx->ptr : nullptr;
      if (m_left > 0) {
        if (kind == CHQ_JOIN_INNER) check_hip(launch_join_expand(ep, ctx.stream), "launch join_expand_kernel");
        else check_hip(launch_join_expand_kind(ep, !left_only, ctx.stream), "launch join_expand_kind_kernel");
        ++ctx.stats.launches;
        if (left_only) { t.read += m_left * 4; t.written += m_left * 4; }
        else { t.read += m_left * 12 + (perm ? m_left * 4 : 0); t.written += m_left * 8; }
      }
      if (u64 > 0) {
        tp.m_left = m_left; tp.m = M; tp.lidx = ep.lidx; tp.ridx = ep.ridx;
        check_hip(launch_join_tail_write(tp, ctx.stream), "launch join_tail_write_kernel");
        ++ctx.stats.launches;
        t.read += nR * 4 + (int64_t)u64 * 4; t.written += (int64_t)u64 * 8;
      }
    }
  }
  ctx.stats.rows_out = M;

  // ---- 7. every left column, then (but for SEMI and ANTI) every right column, through the row-id lists
  const size_t nc = L.cols.size() + (left_only ? 0 : R.cols.size());
  BufferPtr ones = make_device_buffer(nc * 8 + 16, ctx.device);
  check_hip(hipMemsetAsync(ones->ptr, 0, nc * 8 + 16, ctx.stream), "hipMemsetAsync");
  Batch out;
  out.nrows = M; out.on_device = true; out.device_id = ctx.device;
  for (size_t ci = 0; ci < nc; ++ci) {
    const bool is_left = ci < L.cols.size();
    const Column& c = is_left ? L.cols[ci] : R.cols[ci - L.cols.size()];
    const BufferPtr& idx = is_left ? lidx : ridx;
    out.cols.push_back(gather_column(ctx, c, idx ? (const uint32_t*)idx->ptr : nullptr, M, (uint64_t*)ones->ptr + ci, t, is_left ? pad_left : pad_right));
  }
  fill_null_counts(out.cols, M, finish_call(ctx, ones->ptr, nc, t));
  return out;
}

}  // namespace

Batch join_records(Context& ctx, std::vector<Batch>& left, const chq_table_aliases* left_aliases, std::vector<Batch>& right,
                   const chq_table_aliases* right_aliases, const std::vector<JoinKeyArg>& keys, int kind) {
  if (kind < CHQ_JOIN_INNER || kind > CHQ_JOIN_LEFT_ANTI)
    throw ChqError{CHQ_ERR_ARROW_INVALID_ARGUMENT, "unknown join kind " + std::to_string(kind) + " (a chq_join_kind is expected)"};
  if (left.empty() || right.empty()) throw ChqError{CHQ_ERR_ARROW_INVALID_ARGUMENT, "at least one record batch per side is needed"};
  if (keys.empty())
    throw ChqError{CHQ_ERR_ARROW_INVALID_ARGUMENT, "a join needs at least one pair of key columns (there is no cross join)"};
  int64_t rows_l = 0, rows_r = 0;
  for (const Batch& b : left) rows_l += b.nrows;
  for (const Batch& b : right) rows_r += b.nrows;
  if (rows_l + rows_r >= kMaxJoinRows)
    throw ChqError{CHQ_ERR_NOT_SUPPORTED, "a join takes fewer than 2^32 rows per call, both sides together (" + std::to_string(rows_l) + " + " +
                                          std::to_string(rows_r) + " given)"};
  // ---- 1. keys resolve and type-check against both schemas before any data moves, in the caller's terms whatever the kind
  const auto pcols_l = plan_columns(left[0], left_aliases);
  const auto pcols_r = plan_columns(right[0], right_aliases);
  std::vector<int> cols_l, cols_r;
  std::vector<std::string> key_names;
  for (const JoinKeyArg& k : keys) {
    const int cl = resolve_join_key(k.left, "left", pcols_l, rows_l), cr = resolve_join_key(k.right, "right", pcols_r, rows_r);
    const Column& a = left[0].cols[(size_t)cl];
    const Column& b = right[0].cols[(size_t)cr];
    if (a.format != b.format)
      throw ChqError{CHQ_ERR_NOT_SUPPORTED, "join keys '" + a.name + "' (Arrow type '" + a.format + "') and '" + b.name + "' (Arrow type '" + b.format +
                                            "') have different types; coercion between key types is not supported in this build"};
    if (!sortable(a))
      throw ChqError{CHQ_ERR_NOT_SUPPORTED, "join keys '" + a.name + "' and '" + b.name + "' have Arrow type '" + a.format +
                                            "', which has no order in this build"};
    cols_l.push_back(cl); cols_r.push_back(cr);
    key_names.push_back(a.name + " = " + b.name);   // (what a message about the concatenated keys names)
  }
  if (kind != CHQ_JOIN_RIGHT) return join_resolved(ctx, left, right, cols_l, cols_r, key_names, kind);
  // RIGHT: LEFT with the sides exchanged, then the caller's left columns back in front
  Batch res = join_resolved(ctx, right, left, cols_r, cols_l, key_names, CHQ_JOIN_LEFT);
  const size_t n_right_cols = right[0].cols.size();
  std::rotate(res.cols.begin(), res.cols.begin() + (std::ptrdiff_t)n_right_cols, res.cols.end());
  return res;
}

}  // namespace chq
