// join.hpp -- INNER JOIN: the sort-merge equi-join of two groups of record batches (join.cpp), on top of the stable sort
// (sort.hpp) and the group heads of GROUP BY (aggregate.hpp).
#pragma once
#include <cstdint>
#include <vector>

#include "aggregate.hpp"
#include "join_device.h"

namespace chq {

// join.hip
hipError_t launch_join_split(const JoinSplitParams& p, hipStream_t stream);
hipError_t launch_join_count(const JoinCountParams& p, hipStream_t stream);
hipError_t launch_join_scan(const JoinScanParams& p, hipStream_t stream);   // tile sums, scan of the sums, offsets: 3 launches
hipError_t launch_join_expand(const JoinExpandParams& p, hipStream_t stream);

// one `left = right` pair as the C ABI hands it over (chq_join_key)
struct JoinKeyArg {
  const Expr* left = nullptr;    // Identifier / CompoundIdentifier over the left schema
  const Expr* right = nullptr;   // ... over the right schema
};

// One row per pair (left row, right row) whose keys are all non-null with equal bit patterns, ascending by left row, then by
// right row (row order of a side: batch order, then row order).  Every left column, then every right column.  Each side is a
// group of batches of one schema, host or device resident.  The result is ONE device batch.  Throws ChqError; DESIGN.md
// section 3.8.
Batch join_records(Context& ctx, std::vector<Batch>& left, const chq_table_aliases* left_aliases, std::vector<Batch>& right,
                   const chq_table_aliases* right_aliases, const std::vector<JoinKeyArg>& keys);

}  // namespace chq
