// aggregate.hpp -- GROUP BY: grouped COUNT / SUM / MIN / MAX / AVG / COUNT(DISTINCT) of a record batch, or of a group of them joined into one
// (aggregate.cpp), on top of the stable sort (sort.hpp).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "aggregate_device.h"
#include "sort.hpp"

namespace chq {

// aggregate.hip
hipError_t launch_agg_heads(const AggHeadsParams& p, hipStream_t stream);
hipError_t launch_agg_head_scan(const AggGroupsParams& p, hipStream_t stream);
hipError_t launch_agg_head_write(const AggGroupsParams& p, hipStream_t stream);
hipError_t launch_agg_reduce(const AggReduceParams& p, hipStream_t stream);   // reduce, then (two tiles or more) fold
hipError_t launch_agg_count_star(const AggCountStarParams& p, hipStream_t stream);
hipError_t launch_agg_distinct(const AggDistinctParams& p, hipStream_t stream);
hipError_t launch_agg_validity(const AggValidityParams& p, hipStream_t stream);

// The pieces of GROUP BY that JOIN (join.cpp) and the window functions (window.cpp) stand on.
// the runs of equal keys among the sorted positions
struct Runs {
  BufferPtr gids, starts, rep;   // run of every position [n]; first position of every run [G + 1]; one row of every run [G]
  int64_t G = 0;
};
// heads -> head scan -> (read back G) -> head write over the columns `cols` of `rec`, read through `perm`; n >= 1.  No
// column: one heads launch that marks position 0, so all rows are one run.
Runs find_runs(Context& ctx, const Batch& rec, const uint32_t* perm, const std::vector<int>& cols, Traffic& t);

// the aggregates with an argument that reduce through the one accumulator, whatever the caller's enum numbers them
// (chq_agg_kind, chq_window_kind; AVG is GROUP BY's alone: the window functions do not take it)
enum AggFn { AGG_FN_COUNT, AGG_FN_SUM, AGG_FN_MIN, AGG_FN_MAX, AGG_FN_AVG };
// what one output item does, decided against the schema before any data moves
struct AggPlan {
  int col = -1;                 // argument column (key column for CHQ_AGG_KEY)
  int op = AO_COUNT;
  int value_kind = AV_SIGNED;
  std::string format = "l";     // output type: Int64 for the counts, the ranking kinds and the integer sums
  DType type = T_I64;
  int width = 8;
};
// `fn` over column `c`; `name` is what a message calls it.  CHQ_ERR_NOT_SUPPORTED where the type has no such aggregate.
AggPlan plan_aggregate(AggFn fn, const char* name, const Column& c);
// a column of m fixed-width values of the plan's output type over `values`, without nulls
Column fixed_column(const std::string& name, const AggPlan& pl, bool nullable, int64_t m, const BufferPtr& values);
// `o` is null where counts[i] (u64, per group or per row: the values that went into the aggregate) is 0: packs the bitmap,
// adds its set bits to *ones and leaves null_count at -1 for fill_null_counts
void validity_from_counts(Context& ctx, Column& o, const BufferPtr& counts, int64_t m, uint64_t* ones, Traffic& t);

// one output column as the C ABI hands it over (chq_agg_item)
struct AggItemArg {
  int kind = 0;                   // chq_agg_kind
  int key_index = -1;             // CHQ_AGG_KEY
  const Expr* column = nullptr;   // the aggregates but COUNT(*): Identifier / CompoundIdentifier
  std::string name;               // output column name
};

// One row per group of the batches of `in` (one schema, host or device resident), ascending by `keys` with nulls last; one
// column per item, in item order.  The result is ONE device batch.  Throws ChqError; DESIGN.md section 3.7.
Batch aggregate_records(Context& ctx, std::vector<Batch>& in, const chq_table_aliases* aliases, const std::vector<const Expr*>& keys,
                        const std::vector<AggItemArg>& items);

}  // namespace chq
