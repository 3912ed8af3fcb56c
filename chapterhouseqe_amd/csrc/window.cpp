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
// The run finder and the aggregate typing restate aggregate.cpp's: GROUP BY's code and launch sequence stay what they are.
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

// temporal types and decimals of up to 8 bytes: MIN / MAX order them as their signed integers (aggregate.cpp)
bool orders_as_signed(const Column& c) {
  const std::string& f = c.format;
  return c.type == T_FIXED_OPAQUE &&
         (f == "tdD" || f == "tts" || f == "ttm" || f == "tdm" || f == "ttu" || f == "ttn" || f.rfind("ts", 0) == 0 ||
          f.rfind("tD", 0) == 0 || (f.rfind("d:", 0) == 0 && c.width <= 8));
}

// what one output item does, decided against the schema before any data moves
struct ItemPlan {
  int col = -1;                 // argument column
  int op = AO_COUNT;
  int value_kind = AV_SIGNED;
  std::string format = "l";     // output type of the ranking kinds and the aggregates
  DType type = T_I64;
  int width = 8;
};

// the typing of chq_aggregate_records (aggregate.cpp: plan_aggregate)
ItemPlan plan_aggregate(const WinItemArg& it, const Column& c) {
  ItemPlan pl;
  const bool is_signed = c.type >= T_I8 && c.type <= T_I64, is_unsigned = c.type >= T_U8 && c.type <= T_U64;
  const bool is_float = c.type == T_F16 || c.type == T_F32 || c.type == T_F64;
  auto unsupported = [&]() {
    return ChqError{CHQ_ERR_NOT_SUPPORTED, std::string(kind_name(it.kind)) + " over column '" + c.name + "' of Arrow type '" + c.format +
                                           "' is not supported in this build"};
  };
  pl.value_kind = is_unsigned ? AV_UNSIGNED : is_float ? AV_FLOAT : AV_SIGNED;
  switch (it.kind) {
    case CHQ_WIN_COUNT:
      pl.op = AO_COUNT;
      break;
    case CHQ_WIN_SUM:
      if (is_signed) { pl.op = AO_SUM_INT; }
      else if (is_unsigned) { pl.op = AO_SUM_INT; pl.format = "L"; pl.type = T_U64; }
      else if (c.type == T_F32 || c.type == T_F64) { pl.op = AO_SUM_FLOAT; pl.format = "g"; pl.type = T_F64; }
      else throw unsupported();
      break;
    default:   // CHQ_WIN_MIN, CHQ_WIN_MAX
      if (!(is_signed || is_unsigned || is_float || orders_as_signed(c))) throw unsupported();
      pl.op = it.kind == CHQ_WIN_MIN ? AO_MIN : AO_MAX;
      pl.format = c.format; pl.type = c.type; pl.width = c.width;
      break;
  }
  return pl;
}

int resolve_column(const Expr* e, const char* what, const std::vector<PlanColumn>& pcols, int64_t rows) {
  if (e->kind != Expr::IDENT && e->kind != Expr::COMPOUND)
    throw ChqError{CHQ_ERR_NOT_SUPPORTED, std::string(what) + " must be a column, not " + (e->text.empty() ? std::string("an expression") : e->text)};
  return resolve_key(*e, pcols, rows);
}

AggKey key_of(const Column& c) {
  AggKey k{};
  k.validity = c.validity && c.null_count != 0 ? c.validity : nullptr;
  k.bit_offset = c.offset;
  k.values = (const uint8_t*)c.values0();
  k.data = c.data;
  k.kind = c.type == T_BOOL ? AK_BOOL : c.type == T_UTF8 ? AK_UTF8 : AK_FIXED;
  k.width = c.width;
  return k;
}

// the runs of equal keys among the sorted positions
struct Runs {
  BufferPtr gids, starts;   // [n], [G + 1]
  int64_t G = 0;
};

// GROUP BY's heads -> scan -> (read back G) -> write over `cols` (aggregate.cpp); n >= 1
Runs find_runs(Context& ctx, const Batch& rec, const uint32_t* perm, const std::vector<int>& cols, Traffic& t) {
  const int64_t n = rec.nrows, ntiles = (n + kAggTile - 1) / kAggTile;
  Runs r;
  BufferPtr heads = make_device_buffer((size_t)ntiles * kAggTile + 16, ctx.device);
  BufferPtr counts = make_device_buffer((size_t)(ntiles + 1) * 4 + 16, ctx.device);
  AggHeadsParams hp{};
  hp.perm = perm; hp.n = n; hp.heads = (uint8_t*)heads->ptr; hp.tile_counts = (uint32_t*)counts->ptr; hp.ntiles = ntiles;
  size_t k0 = 0;
  do {   // (no key: one launch that marks position 0)
    hp.n_keys = (int32_t)std::min<size_t>(kAggMaxKeys, cols.size() - k0);
    hp.accumulate = k0 ? 1 : 0;
    for (int q = 0; q < hp.n_keys; ++q) {
      const Column& c = rec.cols[(size_t)cols[k0 + (size_t)q]];
      hp.keys[q] = key_of(c);
      t.read += n * (c.type == T_UTF8 ? 8 + (c.length ? std::max<int64_t>(c.data_bytes, 0) / c.length : 0) : std::max(1, c.width));
    }
    check_hip(launch_agg_heads(hp, ctx.stream), "launch agg_heads_kernel");
    ++ctx.stats.launches;
    t.read += perm ? n * 4 : 0; t.written += n + ntiles * 4;
    k0 += (size_t)hp.n_keys;
  } while (k0 < cols.size());
  AggGroupsParams gp{};
  gp.perm = perm; gp.n = n; gp.heads = (const uint8_t*)heads->ptr; gp.tile_counts = (uint32_t*)counts->ptr; gp.ntiles = ntiles;
  check_hip(launch_agg_head_scan(gp, ctx.stream), "launch agg_head_scan_kernel");
  ++ctx.stats.launches;
  uint32_t g32 = 0;
  check_hip(hipMemcpyAsync(&g32, gp.tile_counts + ntiles, 4, hipMemcpyDeviceToHost, ctx.stream), "read back the run count");
  check_hip(hipStreamSynchronize(ctx.stream), "hipStreamSynchronize");
  r.G = (int64_t)g32;
  if (r.G < 1 || r.G > n) throw ChqError{CHQ_ERR_DEVICE, "internal error: " + std::to_string(r.G) + " runs over " + std::to_string(n) + " rows"};
  r.gids = make_device_buffer((size_t)n * 4 + 16, ctx.device);
  r.starts = make_device_buffer((size_t)(r.G + 1) * 4 + 16, ctx.device);
  BufferPtr rep = make_device_buffer((size_t)r.G * 4 + 16, ctx.device);
  gp.gids = (uint32_t*)r.gids->ptr; gp.starts = (uint32_t*)r.starts->ptr; gp.rep = (uint32_t*)rep->ptr; gp.G = r.G;
  check_hip(launch_agg_head_write(gp, ctx.stream), "launch agg_head_write_kernel");
  ++ctx.stats.launches;
  t.read += ntiles * 8 + n + (perm ? r.G * 4 : 0); t.written += ntiles * 4 + n * 4 + r.G * 8;
  return r;
}

Column fixed_column(const std::string& name, const ItemPlan& pl, bool nullable, int64_t n, const BufferPtr& values) {
  Column o;
  o.name = name; o.format = pl.format; o.type = pl.type; o.width = pl.width; o.nullable = nullable;
  o.length = n; o.offset = 0; o.null_count = 0;
  o.values = (const uint8_t*)values->ptr;
  o.owned.push_back(values);
  return o;
}

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
    const int c = resolve_column(e, what, pcols, rows);
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
  std::vector<ItemPlan> plans(ni);
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
      plans[i].col = resolve_column(it.column, (std::string("the argument of ") + kind_name(it.kind)).c_str(), pcols, rows);
      continue;
    }
    if (it.frame < CHQ_FRAME_PARTITION || it.frame > CHQ_FRAME_RANGE_TO_CURRENT)
      throw ChqError{CHQ_ERR_ARROW_INVALID_ARGUMENT, "unknown window frame " + std::to_string(it.frame) + " of output column '" + it.name + "'"};
    need_peers |= it.frame == CHQ_FRAME_RANGE_TO_CURRENT;
    if (it.kind == CHQ_WIN_COUNT_STAR) continue;
    const int col = resolve_column(it.column, (std::string("the argument of ") + kind_name(it.kind)).c_str(), pcols, rows);
    plans[i] = plan_aggregate(it, in[0].cols[(size_t)col]);
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
    const ItemPlan& pl = plans[i];
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
    BufferPtr bits = make_device_buffer((size_t)((n + 31) / 32) * 4 + 16, ctx.device);
    AggValidityParams vp{(const uint64_t*)cnt->ptr, n, (uint8_t*)bits->ptr, ones + nc + i};
    if (n > 0) { check_hip(launch_agg_validity(vp, ctx.stream), "launch agg_validity_kernel"); ++ctx.stats.launches; }
    t.read += n * 8; t.written += (n + 7) / 8;
    o.validity = (const uint8_t*)bits->ptr;
    o.owned.push_back(bits);
    o.null_count = -1;   // set from `ones` once read back
    out.cols.push_back(std::move(o));
  }
  kernel_span_end(ctx);
  // ---- 6. ONE read-back: null counts and overflow flags
  std::vector<uint64_t> h(nc + 2 * ni);
  check_hip(hipMemcpyAsync(h.data(), words->ptr, h.size() * 8, hipMemcpyDeviceToHost, ctx.stream), "read back null counts and overflow flags");
  check_hip(hipStreamSynchronize(ctx.stream), "hipStreamSynchronize");
  ctx.stats.kernel_ns += kernel_span_ns(ctx);
  ctx.stats.bytes_read_alg = t.read; ctx.stats.bytes_written_alg = t.written;
  for (size_t i = 0; i < ni; ++i)
    if (h[nc + ni + i])
      throw ChqError{CHQ_ERR_ARROW_ARITHMETIC_OVERFLOW, "SUM over column '" + rec.cols[(size_t)plans[i].col].name + "' for output column '" +
                                                        items[i].name + "' overflows " + (plans[i].type == T_U64 ? "UInt64" : "Int64") +
                                                        " in the frame of some row"};
  for (size_t ci = 0; ci < out.cols.size(); ++ci)
    if (out.cols[ci].null_count < 0) out.cols[ci].null_count = n - (int64_t)h[ci];
  return out;
}

}  // namespace chq
