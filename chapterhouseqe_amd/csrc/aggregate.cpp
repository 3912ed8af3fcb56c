// aggregate.cpp -- GROUP BY on the device (chq_aggregate_record / chq_aggregate_records).
//
// The stable sort of sort.cpp orders the rows by the keys (every key ascending, nulls last): a group is then a run of
// consecutive sorted positions, and the groups come out in key order.  The kernels of aggregate.hip mark where a run begins,
// number the runs and reduce every aggregate over them, reading the values through the permutation -- no column is gathered
// but the key columns, and those only at one representative row per group.  Two read-backs besides the sort's: the number
// of groups (it sizes the outputs), and one block of null counts and overflow flags at the end.  DESIGN.md section 3.7.
#include <algorithm>
#include <cstring>
#include <string>

#include "aggregate.hpp"

namespace chq {
namespace {

constexpr int64_t kMaxAggRows = (int64_t)1 << 32;   // sorted positions and row ids are u32

const char* kind_name(int kind) {
  switch (kind) {
    case CHQ_AGG_COUNT: return "COUNT";
    case CHQ_AGG_SUM: return "SUM";
    case CHQ_AGG_MIN: return "MIN";
    case CHQ_AGG_MAX: return "MAX";
    default: return "aggregate";
  }
}

// temporal types and decimals of up to 8 bytes: MIN / MAX order them as their signed integers (sort.cpp: key_words)
bool orders_as_signed(const Column& c) {
  const std::string& f = c.format;
  return c.type == T_FIXED_OPAQUE &&
         (f == "tdD" || f == "tts" || f == "ttm" || f == "tdm" || f == "ttu" || f == "ttn" || f.rfind("ts", 0) == 0 ||
          f.rfind("tD", 0) == 0 || (f.rfind("d:", 0) == 0 && c.width <= 8));
}

// what one output item does, decided against the schema before any data moves
struct ItemPlan {
  int col = -1;                 // input column (key column for CHQ_AGG_KEY)
  int op = AO_COUNT;
  int value_kind = AV_SIGNED;
  std::string format;           // output type
  DType type = T_I64;
  int width = 8;
};

ItemPlan plan_aggregate(const AggItemArg& it, const Column& c) {
  ItemPlan pl;
  const bool is_signed = c.type >= T_I8 && c.type <= T_I64, is_unsigned = c.type >= T_U8 && c.type <= T_U64;
  const bool is_float = c.type == T_F16 || c.type == T_F32 || c.type == T_F64;
  auto unsupported = [&]() {
    return ChqError{CHQ_ERR_NOT_SUPPORTED, std::string(kind_name(it.kind)) + " over column '" + c.name + "' of Arrow type '" + c.format +
                                           "' is not supported in this build"};
  };
  pl.value_kind = is_unsigned ? AV_UNSIGNED : is_float ? AV_FLOAT : AV_SIGNED;
  switch (it.kind) {
    case CHQ_AGG_COUNT:
      pl.op = AO_COUNT; pl.format = "l"; pl.type = T_I64; pl.width = 8;
      break;
    case CHQ_AGG_SUM:
      if (is_signed) { pl.op = AO_SUM_INT; pl.format = "l"; pl.type = T_I64; }
      else if (is_unsigned) { pl.op = AO_SUM_INT; pl.format = "L"; pl.type = T_U64; }
      else if (c.type == T_F32 || c.type == T_F64) { pl.op = AO_SUM_FLOAT; pl.format = "g"; pl.type = T_F64; }
      else throw unsupported();
      pl.width = 8;
      break;
    case CHQ_AGG_MIN: case CHQ_AGG_MAX:
      if (!(is_signed || is_unsigned || is_float || orders_as_signed(c))) throw unsupported();
      pl.op = it.kind == CHQ_AGG_MIN ? AO_MIN : AO_MAX;
      pl.format = c.format; pl.type = c.type; pl.width = c.width;
      break;
    default: throw ChqError{CHQ_ERR_ARROW_INVALID_ARGUMENT, "unknown aggregate kind " + std::to_string(it.kind)};
  }
  return pl;
}

int resolve_argument(const AggItemArg& it, const std::vector<PlanColumn>& pcols, int64_t rows) {
  if (!it.column) throw ChqError{CHQ_ERR_INVALID_HANDLE, std::string("null column of ") + kind_name(it.kind)};
  const Expr& e = *it.column;
  if (e.kind != Expr::IDENT && e.kind != Expr::COMPOUND)
    throw ChqError{CHQ_ERR_NOT_SUPPORTED, std::string("the argument of ") + kind_name(it.kind) + " must be a column, not " +
                                          (e.text.empty() ? std::string("an expression") : e.text)};
  return resolve_key(e, pcols, rows);
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

Column fixed_column(const std::string& name, const ItemPlan& pl, bool nullable, int64_t G, const BufferPtr& values) {
  Column o;
  o.name = name; o.format = pl.format; o.type = pl.type; o.width = pl.width; o.nullable = nullable;
  o.length = G; o.offset = 0; o.null_count = 0;
  o.values = (const uint8_t*)values->ptr;
  o.owned.push_back(values);
  return o;
}

}  // namespace

Batch aggregate_records(Context& ctx, std::vector<Batch>& in, const chq_table_aliases* aliases, const std::vector<const Expr*>& keys,
                        const std::vector<AggItemArg>& items) {
  if (in.empty()) throw ChqError{CHQ_ERR_ARROW_INVALID_ARGUMENT, "at least one record batch is needed"};
  if (items.empty()) throw ChqError{CHQ_ERR_ARROW_INVALID_ARGUMENT, "GROUP BY needs at least one output item"};
  int64_t rows = 0;
  for (const Batch& b : in) rows += b.nrows;
  if (rows >= kMaxAggRows)
    throw ChqError{CHQ_ERR_NOT_SUPPORTED, "GROUP BY takes fewer than 2^32 rows per call (" + std::to_string(rows) + " given)"};
  // keys and items resolve against the schema before any data moves
  const auto pcols = plan_columns(in[0], aliases);
  std::vector<int> key_cols;
  std::vector<SortKeyArg> sort_keys;
  for (const Expr* k : keys) {
    if (!k) throw ChqError{CHQ_ERR_INVALID_HANDLE, "null GROUP BY key"};
    key_cols.push_back(resolve_key(*k, pcols, rows));
    sort_keys.push_back(SortKeyArg{k, false, false});
  }
  std::vector<ItemPlan> plans(items.size());
  for (size_t i = 0; i < items.size(); ++i) {
    const AggItemArg& it = items[i];
    if (it.kind == CHQ_AGG_KEY) {
      if (it.key_index < 0 || (size_t)it.key_index >= keys.size())
        throw ChqError{CHQ_ERR_ARROW_INVALID_ARGUMENT, "output column '" + it.name + "' names key " + std::to_string(it.key_index) + " of " +
                                                       std::to_string(keys.size())};
      plans[i].col = key_cols[(size_t)it.key_index];
    } else if (it.kind == CHQ_AGG_COUNT_STAR) {
      plans[i].format = "l";
    } else {
      if (it.kind < CHQ_AGG_COUNT || it.kind > CHQ_AGG_MAX)
        throw ChqError{CHQ_ERR_ARROW_INVALID_ARGUMENT, "unknown aggregate kind " + std::to_string(it.kind)};
      const int col = resolve_argument(it, pcols, rows);
      plans[i] = plan_aggregate(it, in[0].cols[(size_t)col]);
      plans[i].col = col;
    }
  }

  ctx.stats = chq_call_stats{};
  const Batch rec = join_group(ctx, in);
  const int64_t n = rec.nrows, ntiles = (n + kAggTile - 1) / kAggTile;
  ctx.stats.rows_in = n; ctx.stats.tiles = ntiles;
  kernel_span_begin(ctx);
  Traffic t;
  const BufferPtr perm_buf = sort_permutation(ctx, rec, key_cols, sort_keys, t);
  const uint32_t* perm = perm_buf ? (const uint32_t*)perm_buf->ptr : nullptr;

  // ---- the groups: heads -> scan -> (read back G) -> ids, starts, representatives
  int64_t G = 0;
  BufferPtr gids, starts, rep;
  if (n == 0) {
    G = keys.empty() ? 1 : 0;   // no key: one group over no rows
    starts = make_device_buffer((size_t)(G + 1) * 4 + 16, ctx.device);
    check_hip(hipMemsetAsync(starts->ptr, 0, (size_t)(G + 1) * 4, ctx.stream), "hipMemsetAsync");
  } else {
    BufferPtr heads = make_device_buffer((size_t)ntiles * kAggTile + 16, ctx.device);
    BufferPtr counts = make_device_buffer((size_t)(ntiles + 1) * 4 + 16, ctx.device);
    AggHeadsParams hp{};
    hp.perm = perm; hp.n = n; hp.heads = (uint8_t*)heads->ptr; hp.tile_counts = (uint32_t*)counts->ptr; hp.ntiles = ntiles;
    size_t k0 = 0;
    do {   // (no key: one launch that marks position 0)
      hp.n_keys = (int32_t)std::min<size_t>(kAggMaxKeys, key_cols.size() - k0);
      hp.accumulate = k0 ? 1 : 0;
      for (int q = 0; q < hp.n_keys; ++q) {
        const Column& c = rec.cols[(size_t)key_cols[k0 + (size_t)q]];
        hp.keys[q] = key_of(c);
        t.read += n * (c.type == T_UTF8 ? 8 + (c.length ? std::max<int64_t>(c.data_bytes, 0) / c.length : 0) : std::max(1, c.width));
      }
      check_hip(launch_agg_heads(hp, ctx.stream), "launch agg_heads_kernel");
      ++ctx.stats.launches;
      t.read += perm ? n * 4 : 0; t.written += n + ntiles * 4;
      k0 += (size_t)hp.n_keys;
    } while (k0 < key_cols.size());
    AggGroupsParams gp{};
    gp.perm = perm; gp.n = n; gp.heads = (const uint8_t*)heads->ptr; gp.tile_counts = (uint32_t*)counts->ptr; gp.ntiles = ntiles;
    check_hip(launch_agg_head_scan(gp, ctx.stream), "launch agg_head_scan_kernel");
    ++ctx.stats.launches;
    uint32_t g32 = 0;
    check_hip(hipMemcpyAsync(&g32, gp.tile_counts + ntiles, 4, hipMemcpyDeviceToHost, ctx.stream), "read back the group count");
    check_hip(hipStreamSynchronize(ctx.stream), "hipStreamSynchronize");
    G = (int64_t)g32;
    if (G < 1 || G > n) throw ChqError{CHQ_ERR_DEVICE, "internal error: " + std::to_string(G) + " groups over " + std::to_string(n) + " rows"};
    gids = make_device_buffer((size_t)n * 4 + 16, ctx.device);
    starts = make_device_buffer((size_t)(G + 1) * 4 + 16, ctx.device);
    rep = make_device_buffer((size_t)G * 4 + 16, ctx.device);
    gp.gids = (uint32_t*)gids->ptr; gp.starts = (uint32_t*)starts->ptr; gp.rep = (uint32_t*)rep->ptr; gp.G = G;
    check_hip(launch_agg_head_write(gp, ctx.stream), "launch agg_head_write_kernel");
    ++ctx.stats.launches;
    t.read += ntiles * 8 + n + (perm ? G * 4 : 0); t.written += ntiles * 4 + n * 4 + G * 8;
  }
  ctx.stats.rows_out = G;

  // ---- one output column per item
  // words[i]: set validity bits of item i (null_count = G - words[i]); words[items + i]: its overflow flag
  const size_t ni = items.size();
  BufferPtr words = make_device_buffer(ni * 16 + 16, ctx.device);
  check_hip(hipMemsetAsync(words->ptr, 0, ni * 16, ctx.stream), "hipMemsetAsync");
  BufferPtr part_first, part_last;
  Batch out;
  out.nrows = G; out.on_device = true; out.device_id = ctx.device;
  for (size_t i = 0; i < ni; ++i) {
    const AggItemArg& it = items[i];
    const ItemPlan& pl = plans[i];
    uint64_t* ones = (uint64_t*)words->ptr + i;
    if (it.kind == CHQ_AGG_KEY) {
      Column o = gather_column(ctx, rec.cols[(size_t)pl.col], rep ? (const uint32_t*)rep->ptr : nullptr, G, ones, t);
      o.name = it.name;
      out.cols.push_back(std::move(o));
      continue;
    }
    const Column* c = pl.col >= 0 ? &rec.cols[(size_t)pl.col] : nullptr;
    const bool nulls = c && c->validity && c->null_count != 0;
    BufferPtr values = make_device_buffer((size_t)(G * pl.width) + 16, ctx.device);
    if (it.kind == CHQ_AGG_COUNT_STAR || (it.kind == CHQ_AGG_COUNT && !nulls)) {   // the group's rows
      AggCountStarParams cp{(const uint32_t*)starts->ptr, G, (int64_t*)values->ptr};
      if (G > 0) { check_hip(launch_agg_count_star(cp, ctx.stream), "launch agg_count_star_kernel"); ++ctx.stats.launches; }
      t.read += G * 4; t.written += G * 8;
      out.cols.push_back(fixed_column(it.name, pl, false, G, values));
      continue;
    }
    BufferPtr cnt = make_device_buffer((size_t)G * 8 + 16, ctx.device);
    if (n == 0) {   // (G is 0 or 1: a group without rows counts 0 and every other aggregate of it is null)
      check_hip(hipMemsetAsync(values->ptr, 0, (size_t)(G * pl.width) + 16, ctx.stream), "hipMemsetAsync");
      check_hip(hipMemsetAsync(cnt->ptr, 0, (size_t)G * 8 + 16, ctx.stream), "hipMemsetAsync");
    } else {
      if (!part_first) {
        part_first = make_device_buffer((size_t)ntiles * sizeof(AggAcc) + 16, ctx.device);
        part_last = make_device_buffer((size_t)ntiles * sizeof(AggAcc) + 16, ctx.device);
      }
      AggReduceParams rp{};
      rp.perm = perm; rp.n = n; rp.ntiles = ntiles; rp.gids = (const uint32_t*)gids->ptr; rp.starts = (const uint32_t*)starts->ptr; rp.G = G;
      rp.values = pl.op == AO_COUNT ? nullptr : (const uint8_t*)c->values0();
      rp.validity = nulls ? c->validity : nullptr;
      rp.bit_offset = c->offset;
      rp.part_first = (AggAcc*)part_first->ptr; rp.part_last = (AggAcc*)part_last->ptr;
      rp.out = (uint8_t*)values->ptr; rp.cnt_out = pl.op == AO_COUNT ? nullptr : (uint64_t*)cnt->ptr;
      rp.overflow = (uint32_t*)((uint64_t*)words->ptr + ni + i);
      rp.op = pl.op; rp.value_kind = pl.value_kind; rp.width = c->width;
      check_hip(launch_agg_reduce(rp, ctx.stream), "launch agg_reduce_kernel");
      ctx.stats.launches += ntiles > 1 ? 2 : 1;
      t.read += n * 4 + (perm ? n * 4 : 0) + (nulls ? (n + 7) / 8 : 0) + (pl.op == AO_COUNT ? 0 : n * c->width) + G * 8;
      t.written += G * (pl.width + 8) + ntiles * 2 * (int64_t)sizeof(AggAcc);
    }
    if (pl.op == AO_COUNT) {
      out.cols.push_back(fixed_column(it.name, pl, false, G, values));
      continue;
    }
    Column o = fixed_column(it.name, pl, true, G, values);
    BufferPtr bits = make_device_buffer((size_t)((G + 31) / 32) * 4 + 16, ctx.device);
    AggValidityParams vp{(const uint64_t*)cnt->ptr, G, (uint8_t*)bits->ptr, ones};
    if (G > 0) { check_hip(launch_agg_validity(vp, ctx.stream), "launch agg_validity_kernel"); ++ctx.stats.launches; }
    t.read += G * 8; t.written += (G + 7) / 8;
    o.validity = (const uint8_t*)bits->ptr;
    o.owned.push_back(bits);
    o.null_count = -1;   // set from `ones` once read back
    out.cols.push_back(std::move(o));
  }
  kernel_span_end(ctx);
  std::vector<uint64_t> h(ni * 2);
  check_hip(hipMemcpyAsync(h.data(), words->ptr, ni * 16, hipMemcpyDeviceToHost, ctx.stream), "read back null counts and overflow flags");
  check_hip(hipStreamSynchronize(ctx.stream), "hipStreamSynchronize");
  ctx.stats.kernel_ns += kernel_span_ns(ctx);
  ctx.stats.bytes_read_alg = t.read; ctx.stats.bytes_written_alg = t.written;
  for (size_t i = 0; i < ni; ++i) {
    if (h[ni + i])
      throw ChqError{CHQ_ERR_ARROW_ARITHMETIC_OVERFLOW, "SUM over column '" + rec.cols[(size_t)plans[i].col].name + "' for output column '" +
                                                        items[i].name + "' overflows " + (plans[i].type == T_U64 ? "UInt64" : "Int64")};
    if (out.cols[i].null_count < 0) out.cols[i].null_count = G - (int64_t)h[i];
  }
  return out;
}

}  // namespace chq
