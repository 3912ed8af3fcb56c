// aggregate.hpp -- GROUP BY: grouped COUNT / SUM / MIN / MAX of a record batch, or of a group of them joined into one
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
hipError_t launch_agg_validity(const AggValidityParams& p, hipStream_t stream);

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
