// window.cpp -- window functions on the device (chq_window_record / chq_window_records).
//
// ONE stable sort by the partition keys (ascending, nulls last), then the order keys, serves every item of the call; ONE
// run of GROUP BY's heads -> scan -> write kernels over the partition keys gives the partitions, and -- only when an item
// needs peers -- one more over partition and order keys the peer groups.  The kernels of window.hip then work on sorted
// positions and write every result to the row's place in INPUT order, so no column is permuted: the input columns are
// copied through the identity gather, LAG / LEAD are the outer joins' null-producing gather through a shifted row list.
// Read-backs besides the sort's and the gathers': the partitions, the peer groups when needed, and ONE block of null
// counts and overflow flags at the end.  DESIGN.md section 3.10.
//
// The run finder (find_runs) and the typing of the aggregates (plan_aggregate) are GROUP BY's own: aggregate.hpp.
#include <algorithm>
#include <cstring>
#include <string>

#include "window.hpp"

namespace chq {
namespace {

constexpr int64_t kMaxWinRows = (int64_t)1 << 32;   // sorted positions and row ids are u32

const char* kind_name(int kind) {
  switch (kind) {
    case CHQ_WIN_ROW_NUMBER: return "ROW_NUMBER";
    case CHQ_WIN_RANK: return "RANK";
    case CHQ_WIN_DENSE_RANK: return "DENSE_RANK";
    case CHQ_WIN_LAG: return "LAG";
    case CHQ_WIN_LEAD: return "LEAD";
    case CHQ_WIN_COUNT_STAR: case CHQ_WIN_COUNT: return "COUNT";
    case CHQ_WIN_SUM: return "SUM";
    case CHQ_WIN_MIN: return "MIN";
    case CHQ_WIN_MAX: return "MAX";
    default: return "window function";
  }
}

bool is_ranking(int kind) { return kind >= CHQ_WIN_ROW_NUMBER && kind <= CHQ_WIN_DENSE_RANK; }
bool is_shift(int kind) { return kind == CHQ_WIN_LAG || kind == CHQ_WIN_LEAD; }
bool needs_column(int kind) { return is_shift(kind) || (kind >= CHQ_WIN_COUNT && kind <= CHQ_WIN_MAX); }

static_assert(CHQ_WIN_SUM - CHQ_WIN_COUNT == AGG_FN_SUM && CHQ_WIN_MIN - CHQ_WIN_COUNT == AGG_FN_MIN && CHQ_WIN_MAX - CHQ_WIN_COUNT == AGG_FN_MAX,
              "chq_window_kind numbers COUNT, SUM, MIN, MAX like AggFn");

}  // namespace

Batch window_records(Context& ctx, std::vector<Batch>& in, const chq_table_aliases* aliases, const std::vector<const Expr*>& partition_by,
                     const std::vector<SortKeyArg>& order_by, const std::vector<WinItemArg>& items) {
  if (in.empty()) throw ChqError{CHQ_ERR_ARROW_INVALID_ARGUMENT, "at least one record batch is needed"};
  if (items.empty()) throw ChqError{CHQ_ERR_ARROW_INVALID_ARGUMENT, "a window call needs at least one item"};
  int64_t rows = 0;
  for (const Batch& b : in) rows += b.nrows;
  if (rows >= kMaxWinRows)
    throw ChqError{CHQ_ERR_NOT_SUPPORTED, "a window call takes fewer than 2^32 rows (" + std::to_string(rows) + " given)"};
  // ---- 1. keys and items resolve and type-check against the schema before any data moves
  const auto pcols = plan_columns(in[0], aliases);
  std::vector<int> key_cols;          // partition keys, then order keys
  std::vector<SortKeyArg> sort_keys;
  auto add_key = [&](const Expr* e, const char* what, bool descending, bool nulls_first) {
    if (!e) throw ChqError{CHQ_ERR_INVALID_HANDLE, std::string("null ") + what};
    const int c = resolve_key(*e, pcols, rows, what);
    const Column& col = in[0].cols[(size_t)c];
    if (!sortable(col))
      throw ChqError{CHQ_ERR_NOT_SUPPORTED, std::string(what) + " '" + col.name + "' has Arrow type '" + col.format + "', which has no order in this build"};
    key_cols.push_back(c);
    sort_keys.push_back(SortKeyArg{e, descending, nulls_first});
  };
  for (const Expr* e : partition_by) add_key(e, "a PARTITION BY key", false, false);
  for (const SortKeyArg& k : order_by) add_key(k.column, "an ORDER BY key", k.descending, k.nulls_first);
  const std::vector<int> part_cols(key_cols.begin(), key_cols.begin() + (std::ptrdiff_t)partition_by.size());

  const size_t ni = items.size();
  std::vector<AggPlan> plans(ni);
  bool need_peers = false;
  for (size_t i = 0; i < ni; ++i) {
    const WinItemArg& it = items[i];
    if (it.kind < CHQ_WIN_ROW_NUMBER || it.kind > CHQ_WIN_MAX)
      throw ChqError{CHQ_ERR_ARROW_INVALID_ARGUMENT, "unknown window function kind " + std::to_string(it.kind) + " of output column '" + it.name + "'"};
    if (needs_column(it.kind) && !it.column)
      throw ChqError{CHQ_ERR_ARROW_INVALID_ARGUMENT, std::string(kind_name(it.kind)) + " for output column '" + it.name + "' needs a column"};
    if (is_ranking(it.kind)) {
      need_peers |= it.kind != CHQ_WIN_ROW_NUMBER;
      continue;
    }
    if (is_shift(it.kind)) {
      if (it.offset < 0)
        throw ChqError{CHQ_ERR_ARROW_INVALID_ARGUMENT, std::string(kind_name(it.kind)) + " for output column '" + it.name + "' has the negative offset " +
                                                       std::to_string(it.offset)};
      plans[i].col = resolve_key(*it.column, pcols, rows, std::string("the argument of ") + kind_name(it.kind));
      continue;
    }
    if (it.frame < CHQ_FRAME_PARTITION || it.frame > CHQ_FRAME_RANGE_TO_CURRENT)
      throw ChqError{CHQ_ERR_ARROW_INVALID_ARGUMENT, "unknown window frame " + std::to_string(it.frame) + " of output column '" + it.name + "'"};
    need_peers |= it.frame == CHQ_FRAME_RANGE_TO_CURRENT;
    if (it.kind == CHQ_WIN_COUNT_STAR) continue;
    const int col = resolve_key(*it.column, pcols, rows, std::string("the argument of ") + kind_name(it.kind));
    plans[i] = plan_aggregate((AggFn)(it.kind - CHQ_WIN_COUNT), kind_name(it.kind), in[0].cols[(size_t)col]);
    plans[i].col = col;
  }

  // ---- 2. one device batch, one sort, the partitions and (when needed) the peer groups
  ctx.stats = chq_call_stats{};
  const Batch rec = join_group(ctx, in);
  const int64_t n = rec.nrows, ntiles = (n + kWinTile - 1) / kWinTile;
  ctx.stats.rows_in = n; ctx.stats.rows_out = n; ctx.stats.tiles = ntiles;
  kernel_span_begin(ctx);
  Traffic t;
  const BufferPtr perm_buf = sort_permutation(ctx, rec, key_cols, sort_keys, t);
  const uint32_t* perm = perm_buf ? (const uint32_t*)perm_buf->ptr : nullptr;
  Runs parts, peers;
  if (n > 0) {
    parts = find_runs(ctx, rec, perm, part_cols, t);
    peers = need_peers && !order_by.empty() ? find_runs(ctx, rec, perm, key_cols, t) : parts;   // (no order key: the partition is the peer group)
  }
  const uint32_t* pgid = n > 0 ? (const uint32_t*)parts.gids->ptr : nullptr;
  const uint32_t* pstarts = n > 0 ? (const uint32_t*)parts.starts->ptr : nullptr;
  const uint32_t* qgid = n > 0 ? (const uint32_t*)peers.gids->ptr : nullptr;
  const uint32_t* qstarts = n > 0 ? (const uint32_t*)peers.starts->ptr : nullptr;

  // ---- 3. the input columns, in input order
  // words[c]: set validity bits of output column c (null_count = n - words[c]); words[nc + ni + i]: overflow flag of item i
  const size_t nc = rec.cols.size();
  BufferPtr words = make_device_buffer((nc + 2 * ni) * 8 + 16, ctx.device);
  check_hip(hipMemsetAsync(words->ptr, 0, (nc + 2 * ni) * 8, ctx.stream), "hipMemsetAsync");
  uint64_t* const ones = (uint64_t*)words->ptr;
  Batch out;
  out.nrows = n; out.on_device = true; out.device_id = ctx.device;
  for (size_t ci = 0; ci < nc; ++ci) out.cols.push_back(gather_column(ctx, rec.cols[ci], nullptr, n, ones + ci, t));

  // ---- 4. every ranking item in one launch (items of one kind share their values)
  BufferPtr rank_values[3];
  if (n > 0) {
    WinRankParams rp{};
    rp.perm = perm; rp.n = n; rp.pgid = pgid; rp.pstarts = pstarts; rp.qgid = qgid; rp.qstarts = qstarts;
    int64_t** const slots[3] = {&rp.row_number, &rp.rank, &rp.dense_rank};
    int n_rank = 0;
    for (const WinItemArg& it : items)
      if (is_ranking(it.kind) && !rank_values[it.kind]) {
        rank_values[it.kind] = make_device_buffer((size_t)n * 8 + 16, ctx.device);
        *slots[it.kind] = (int64_t*)rank_values[it.kind]->ptr;
        ++n_rank;
      }
    if (n_rank) {
      check_hip(launch_win_rank(rp, ctx.stream), "launch win_rank_kernel");
      ++ctx.stats.launches;
      t.read += (perm ? n * 4 : 0) + n * 8 + (rp.rank || rp.dense_rank ? n * 4 + (rp.rank ? n * 4 : 0) + (rp.dense_rank ? n * 4 : 0) : 0);
      t.written += n * 8 * n_rank;
    }
  }

  // ---- 5. the other items, one column each
  BufferPtr scan_a, scan_b, scan_cnt, tile_tot, tile_carry;   // the scan's scratch, shared by the items (one stream: one at a time)
  for (size_t i = 0; i < ni; ++i) {
    const WinItemArg& it = items[i];
    const AggPlan& pl = plans[i];
    if (is_ranking(it.kind)) {
      const BufferPtr values = n > 0 ? rank_values[it.kind] : make_device_buffer(16, ctx.device);
      out.cols.push_back(fixed_column(it.name, pl, false, n, values));
      continue;
    }
    if (is_shift(it.kind)) {
      BufferPtr src = make_device_buffer((size_t)n * 4 + 16, ctx.device);
      if (n > 0) {
        WinShiftParams sp{};
        sp.perm = perm; sp.n = n; sp.pgid = pgid; sp.pstarts = pstarts; sp.src = (uint32_t*)src->ptr;
        const int64_t off = std::min<int64_t>(it.offset, kMaxWinRows);   // (past every partition anyway)
        sp.delta = it.kind == CHQ_WIN_LAG ? -off : off;
        check_hip(launch_win_shift(sp, ctx.stream), "launch win_shift_kernel");
        ++ctx.stats.launches;
        t.read += (perm ? n * 8 : 0) + n * 12; t.written += n * 4;
      }
      Column o = gather_column(ctx, rec.cols[(size_t)pl.col], (const uint32_t*)src->ptr, n, ones + nc + i, t, true);
      o.name = it.name;
      out.cols.push_back(std::move(o));
      continue;
    }
    const Column* c = pl.col >= 0 ? &rec.cols[(size_t)pl.col] : nullptr;
    const bool nulls = c && c->validity && c->null_count != 0;
    const bool rows_only = it.kind == CHQ_WIN_COUNT_STAR || (it.kind == CHQ_WIN_COUNT && !nulls);   // the count is the frame's rows
    BufferPtr values = make_device_buffer((size_t)(n * pl.width) + 16, ctx.device);
    BufferPtr cnt = pl.op == AO_COUNT ? nullptr : make_device_buffer((size_t)n * 8 + 16, ctx.device);
    if (n > 0) {
      WinAggParams ap{};
      ap.perm = perm; ap.n = n; ap.ntiles = ntiles; ap.pgid = pgid; ap.pstarts = pstarts; ap.qgid = qgid; ap.qstarts = qstarts;
      ap.out = (uint8_t*)values->ptr; ap.cnt_out = cnt ? (uint64_t*)cnt->ptr : nullptr;
      ap.overflow = (uint32_t*)(ones + nc + ni + i);
      ap.op = pl.op; ap.value_kind = pl.value_kind; ap.width = c ? c->width : 8;
      ap.frame = it.frame == CHQ_FRAME_PARTITION ? WF_PARTITION : it.frame == CHQ_FRAME_ROWS_TO_CURRENT ? WF_ROWS : WF_RANGE;
      if (!rows_only) {
        const bool has_a = pl.op != AO_COUNT, has_b = pl.op == AO_SUM_INT;
        if (has_a && !scan_a) scan_a = make_device_buffer((size_t)n * 8 + 16, ctx.device);
        if (has_b && !scan_b) scan_b = make_device_buffer((size_t)n * 8 + 16, ctx.device);
        if (!scan_cnt) {
          scan_cnt = make_device_buffer((size_t)n * 4 + 16, ctx.device);
          tile_tot = make_device_buffer((size_t)ntiles * sizeof(AggAcc) + 16, ctx.device);
          tile_carry = make_device_buffer((size_t)ntiles * sizeof(AggAcc) + 16, ctx.device);
        }
        ap.values = pl.op == AO_COUNT ? nullptr : (const uint8_t*)c->values0();
        ap.validity = nulls ? c->validity : nullptr;
        ap.bit_offset = c->offset;
        ap.scan_a = has_a ? (uint64_t*)scan_a->ptr : nullptr; ap.scan_b = has_b ? (uint64_t*)scan_b->ptr : nullptr;
        ap.scan_cnt = (uint32_t*)scan_cnt->ptr;
        ap.tile_tot = (AggAcc*)tile_tot->ptr; ap.tile_carry = (AggAcc*)tile_carry->ptr;
        check_hip(launch_win_scan(ap, ctx.stream), "launch win_scan_kernel / win_carry_kernel");
        ctx.stats.launches += 2;
        const int64_t elem = 4 + (has_a ? 8 : 0) + (has_b ? 8 : 0);   // bytes of one scanned element
        t.read += n * 4 + (perm ? n * 4 : 0) + (nulls ? (n + 7) / 8 : 0) + (pl.op == AO_COUNT ? 0 : n * c->width) +
                  ntiles * ((int64_t)sizeof(AggAcc) + 8);
        t.written += n * elem + ntiles * 2 * (int64_t)sizeof(AggAcc);
        t.read += n * elem + ntiles * (int64_t)sizeof(AggAcc);   // what the emit launch reads of it
      }
      check_hip(launch_win_emit(ap, ctx.stream), "launch win_emit_kernel");
      ++ctx.stats.launches;
      t.read += (perm ? n * 4 : 0) + n * 8 + (ap.frame == WF_RANGE ? n * 8 : ap.frame == WF_PARTITION ? n * 4 : 0);
      t.written += n * (pl.width + (cnt ? 8 : 0));
    }
    if (pl.op == AO_COUNT) {
      out.cols.push_back(fixed_column(it.name, pl, false, n, values));
      continue;
    }
    // validity: the per-row counts were scattered in input order; the bitmap is packed from them contiguously
    Column o = fixed_column(it.name, pl, true, n, values);
    validity_from_counts(ctx, o, cnt, n, ones + nc + i, t);
    out.cols.push_back(std::move(o));
  }
  // ---- 6. ONE read-back: null counts and overflow flags
  const std::vector<uint64_t> h = finish_call(ctx, words->ptr, nc + 2 * ni, t, "read back null counts and overflow flags");
  for (size_t i = 0; i < ni; ++i)
    if (h[nc + ni + i])
      throw ChqError{CHQ_ERR_ARROW_ARITHMETIC_OVERFLOW, "SUM over column '" + rec.cols[(size_t)plans[i].col].name + "' for output column '" +
                                                        items[i].name + "' overflows " + (plans[i].type == T_U64 ? "UInt64" : "Int64") +
                                                        " in the frame of some row"};
  fill_null_counts(out.cols, n, h);
  return out;
}

}  // namespace chq
