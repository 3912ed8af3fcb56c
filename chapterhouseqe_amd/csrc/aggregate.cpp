// aggregate.cpp -- GROUP BY on the device (chq_aggregate_record / chq_aggregate_records).
//
// The stable sort of sort.cpp orders the rows by the keys (every key ascending, nulls last): a group is then a run of
// consecutive sorted positions, and the groups come out in key order.  The kernels of aggregate.hip mark where a run begins,
// number the runs and reduce every aggregate over them, reading the values through the permutation -- no column is gathered
// but the key columns, and those only at one representative row per group.  Two read-backs besides the sort's: the number
// of groups (it sizes the outputs), and one block of null counts and overflow flags at the end.  COUNT(DISTINCT c) sorts a
// second time, by (keys, c), finds the runs of that order and counts them per group; a call without it does none of that.
// DESIGN.md section 3.7.
//
// The run finder (find_runs) and the typing of the aggregates (plan_aggregate) are defined here for JOIN (join.cpp) and the
// window functions (window.cpp) as well: aggregate.hpp declares them.
#include <algorithm>
#include <cstring>
#include <map>
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
    case CHQ_AGG_AVG: return "AVG";
    case CHQ_AGG_COUNT_DISTINCT: return "COUNT_DISTINCT";
    default: return "aggregate";
  }
}

static_assert(CHQ_AGG_SUM - CHQ_AGG_COUNT == AGG_FN_SUM && CHQ_AGG_MIN - CHQ_AGG_COUNT == AGG_FN_MIN && CHQ_AGG_MAX - CHQ_AGG_COUNT == AGG_FN_MAX &&
              CHQ_AGG_AVG - CHQ_AGG_COUNT == AGG_FN_AVG,
              "chq_agg_kind numbers COUNT, SUM, MIN, MAX, AVG like AggFn");

AggKey key_of(const Column& c) {
  AggKey k{};
  k.validity = c.live_validity();
  k.bit_offset = c.offset;
  k.values = (const uint8_t*)c.values0();
  k.data = c.data;
  k.kind = c.type == T_BOOL ? AK_BOOL : c.type == T_UTF8 ? AK_UTF8 : AK_FIXED;
  k.width = c.width;
  return k;
}

}  // namespace

AggPlan plan_aggregate(AggFn fn, const char* name, const Column& c) {
  AggPlan pl;
  const bool is_signed = c.type >= T_I8 && c.type <= T_I64, is_unsigned = c.type >= T_U8 && c.type <= T_U64;
  const bool is_float = c.type == T_F16 || c.type == T_F32 || c.type == T_F64;
  auto unsupported = [&]() {
    return ChqError{CHQ_ERR_NOT_SUPPORTED, std::string(name) + " over column '" + c.name + "' of Arrow type '" + c.format +
                                           "' is not supported in this build"};
  };
  pl.value_kind = is_unsigned ? AV_UNSIGNED : is_float ? AV_FLOAT : AV_SIGNED;
  switch (fn) {
    case AGG_FN_COUNT:
      pl.op = AO_COUNT;
      break;
    case AGG_FN_SUM:
      if (is_signed) { pl.op = AO_SUM_INT; }
      else if (is_unsigned) { pl.op = AO_SUM_INT; pl.format = "L"; pl.type = T_U64; }
      else if (c.type == T_F32 || c.type == T_F64) { pl.op = AO_SUM_FLOAT; pl.format = "g"; pl.type = T_F64; }
      else throw unsupported();
      break;
    case AGG_FN_MIN: case AGG_FN_MAX:
      if (!(is_signed || is_unsigned || is_float || orders_as_signed(c))) throw unsupported();
      pl.op = fn == AGG_FN_MIN ? AO_MIN : AO_MAX;
      pl.format = c.format; pl.type = c.type; pl.width = c.width;
      break;
    case AGG_FN_AVG:   // the types SUM takes; Float64 whatever the input
      if (is_signed || is_unsigned) pl.op = AO_AVG_INT;
      else if (c.type == T_F32 || c.type == T_F64) pl.op = AO_AVG_FLOAT;
      else throw unsupported();
      pl.format = "g"; pl.type = T_F64;
      break;
  }
  return pl;
}

Column fixed_column(const std::string& name, const AggPlan& pl, bool nullable, int64_t m, const BufferPtr& values) {
  Column o;
  o.name = name; o.format = pl.format; o.type = pl.type; o.width = pl.width; o.nullable = nullable;
  o.length = m; o.offset = 0; o.null_count = 0;
  o.values = (const uint8_t*)values->ptr;
  o.owned.push_back(values);
  return o;
}

void validity_from_counts(Context& ctx, Column& o, const BufferPtr& counts, int64_t m, uint64_t* ones, Traffic& t) {
  BufferPtr bits = make_device_buffer((size_t)((m + 31) / 32) * 4 + 16, ctx.device);
  AggValidityParams vp{(const uint64_t*)counts->ptr, m, (uint8_t*)bits->ptr, ones};
  if (m > 0) { check_hip(launch_agg_validity(vp, ctx.stream), "launch agg_validity_kernel"); ++ctx.stats.launches; }
  t.read += m * 8; t.written += (m + 7) / 8;
  o.validity = (const uint8_t*)bits->ptr;
  o.owned.push_back(bits);
  o.null_count = -1;   // set from `ones` once read back
}

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
  // agg_head_write_kernel writes rep[] without a test: it is allocated for every caller, whether or not that caller reads it
  r.rep = make_device_buffer((size_t)r.G * 4 + 16, ctx.device);
  gp.gids = (uint32_t*)r.gids->ptr; gp.starts = (uint32_t*)r.starts->ptr; gp.rep = (uint32_t*)r.rep->ptr; gp.G = r.G;
  check_hip(launch_agg_head_write(gp, ctx.stream), "launch agg_head_write_kernel");
  ++ctx.stats.launches;
  t.read += ntiles * 8 + n + (perm ? r.G * 4 : 0); t.written += ntiles * 4 + n * 4 + r.G * 8;
  return r;
}

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
  std::vector<AggPlan> plans(items.size());
  for (size_t i = 0; i < items.size(); ++i) {
    const AggItemArg& it = items[i];
    if (it.kind == CHQ_AGG_KEY) {
      if (it.key_index < 0 || (size_t)it.key_index >= keys.size())
        throw ChqError{CHQ_ERR_ARROW_INVALID_ARGUMENT, "output column '" + it.name + "' names key " + std::to_string(it.key_index) + " of " +
                                                       std::to_string(keys.size())};
      plans[i].col = key_cols[(size_t)it.key_index];
    } else if (it.kind != CHQ_AGG_COUNT_STAR) {
      if (it.kind < CHQ_AGG_COUNT || it.kind > CHQ_AGG_COUNT_DISTINCT)
        throw ChqError{CHQ_ERR_ARROW_INVALID_ARGUMENT, "unknown aggregate kind " + std::to_string(it.kind)};
      if (!it.column) throw ChqError{CHQ_ERR_INVALID_HANDLE, std::string("null column of ") + kind_name(it.kind)};
      const int col = resolve_key(*it.column, pcols, rows, std::string("the argument of ") + kind_name(it.kind));
      const Column& c = in[0].cols[(size_t)col];
      if (it.kind == CHQ_AGG_COUNT_DISTINCT) {   // the argument is sorted behind the keys: the types of a key (Int64 out, the default plan)
        if (!sortable(c))
          throw ChqError{CHQ_ERR_NOT_SUPPORTED, "COUNT_DISTINCT over column '" + c.name + "' of Arrow type '" + c.format +
                                                "' is not supported in this build: the type has no order"};
      } else {
        plans[i] = plan_aggregate((AggFn)(it.kind - CHQ_AGG_COUNT), kind_name(it.kind), c);
      }
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

  // ---- the groups: ids, starts, representatives
  Runs runs;
  if (n == 0) {
    runs.G = keys.empty() ? 1 : 0;   // no key: one group over no rows
    runs.starts = make_device_buffer((size_t)(runs.G + 1) * 4 + 16, ctx.device);
    check_hip(hipMemsetAsync(runs.starts->ptr, 0, (size_t)(runs.G + 1) * 4, ctx.stream), "hipMemsetAsync");
  } else {
    runs = find_runs(ctx, rec, perm, key_cols, t);
  }
  const int64_t G = runs.G;
  const BufferPtr &gids = runs.gids, &starts = runs.starts, &rep = runs.rep;
  ctx.stats.rows_out = G;

  // ---- one output column per item
  // words[i]: set validity bits of item i (null_count = G - words[i]); words[items + i]: its overflow flag
  const size_t ni = items.size();
  BufferPtr words = make_device_buffer(ni * 16 + 16, ctx.device);
  check_hip(hipMemsetAsync(words->ptr, 0, ni * 16, ctx.stream), "hipMemsetAsync");
  BufferPtr part_first, part_last;
  std::map<int, Runs> fine_runs;   // COUNT_DISTINCT: the runs of (keys, argument column), by argument column
  Batch out;
  out.nrows = G; out.on_device = true; out.device_id = ctx.device;
  for (size_t i = 0; i < ni; ++i) {
    const AggItemArg& it = items[i];
    const AggPlan& pl = plans[i];
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
    if (it.kind == CHQ_AGG_COUNT_DISTINCT) {
      if (n == 0) {   // (G is 0 or 1: a group without rows has no value)
        check_hip(hipMemsetAsync(values->ptr, 0, (size_t)(G * pl.width) + 16, ctx.stream), "hipMemsetAsync");
      } else {
        // The rows sorted by (keys, c): the sort is stable and the keys come first, so group g keeps its sorted positions
        // [starts[g], starts[g + 1]) and the runs of (keys, c) -- the fine runs -- cut it into its distinct values, nulls
        // last.  One more sort and one more run finding per argument column, shared by the items that name it.
        auto found = fine_runs.find(pl.col);
        if (found == fine_runs.end()) {
          std::vector<int> cols2 = key_cols;
          std::vector<SortKeyArg> keys2 = sort_keys;
          cols2.push_back(pl.col);
          keys2.push_back(SortKeyArg{it.column, false, false});
          const BufferPtr perm2 = sort_permutation(ctx, rec, cols2, keys2, t);
          Runs fine = find_runs(ctx, rec, perm2 ? (const uint32_t*)perm2->ptr : nullptr, cols2, t);
          fine.gids = nullptr;   // 4n bytes that the distinct kernel never reads: only starts and rep stay until the call ends
          found = fine_runs.emplace(pl.col, std::move(fine)).first;
        }
        const Runs& fine = found->second;
        AggDistinctParams dp{};
        dp.starts = (const uint32_t*)starts->ptr; dp.G = G;
        dp.starts2 = (const uint32_t*)fine.starts->ptr; dp.rep2 = (const uint32_t*)fine.rep->ptr; dp.G2 = fine.G;
        dp.validity = nulls ? c->validity : nullptr; dp.bit_offset = c->offset;
        dp.out = (int64_t*)values->ptr;
        check_hip(launch_agg_distinct(dp, ctx.stream), "launch agg_distinct_kernel");
        ++ctx.stats.launches;
        t.read += G * 8 + fine.G * 4 + (nulls ? G * 5 : 0); t.written += G * 8;
      }
      out.cols.push_back(fixed_column(it.name, pl, false, G, values));
      continue;
    }
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
    validity_from_counts(ctx, o, cnt, G, ones, t);
    out.cols.push_back(std::move(o));
  }
  const std::vector<uint64_t> h = finish_call(ctx, words->ptr, ni * 2, t, "read back null counts and overflow flags");
  for (size_t i = 0; i < ni; ++i)
    if (h[ni + i])
      throw ChqError{CHQ_ERR_ARROW_ARITHMETIC_OVERFLOW, "SUM over column '" + rec.cols[(size_t)plans[i].col].name + "' for output column '" +
                                                        items[i].name + "' overflows " + (plans[i].type == T_U64 ? "UInt64" : "Int64")};
  fill_null_counts(out.cols, G, h);
  return out;
}

}  // namespace chq
