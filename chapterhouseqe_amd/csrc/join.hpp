// join.hpp -- JOIN: the sort-merge equi-join of two groups of record batches (join.cpp), on top of the stable sort
// (sort.hpp) and the group heads of GROUP BY (aggregate.hpp).  Kinds: INNER, LEFT, RIGHT, FULL, LEFT_SEMI, LEFT_ANTI.
#pragma once
#include <cstdint>
#include <vector>

#include "aggregate.hpp"
#include "join_device.h"

namespace chq {

// join.hip
hipError_t launch_join_split(const JoinSplitParams& p, hipStream_t stream);
hipError_t launch_join_count(const JoinCountParams& p, hipStream_t stream);
hipError_t launch_join_expand(const JoinExpandParams& p, hipStream_t stream);
// the kinds other than INNER: count with a rule, expand with "no row" (right: LEFT / FULL; else lidx only), FULL's tail
hipError_t launch_join_count_kind(const JoinCountKindParams& p, hipStream_t stream);
hipError_t launch_join_expand_kind(const JoinExpandParams& p, bool right, hipStream_t stream);
hipError_t launch_join_tail_flag(const JoinTailParams& p, hipStream_t stream);
hipError_t launch_join_tail_write(const JoinTailParams& p, hipStream_t stream);

// one `left = right` pair as the C ABI hands it over (chq_join_key)
struct JoinKeyArg {
  const Expr* left = nullptr;    // Identifier / CompoundIdentifier over the left schema
  const Expr* right = nullptr;   // ... over the right schema
};

// INNER: one row per pair (left row, right row) whose keys are all non-null with equal bit patterns, ascending by left row,
// then by right row (row order of a side: batch order, then row order).  Every left column, then every right column.
// LEFT: the same, and a left row without a pair gives one row with every right column null.  RIGHT: LEFT with the sides
// exchanged (ascending by right row, then by left row), columns still left then right.  FULL: the rows of LEFT, then every
// right row without a pair, ascending, with every left column null.  LEFT_SEMI / LEFT_ANTI: every left row with / without a
// pair, once, ascending; left columns only.  The fields of a padded side come out nullable.  `kind` is a chq_join_kind; any
// other value: CHQ_ERR_ARROW_INVALID_ARGUMENT.  Each side is a group of batches of one schema, host or device resident.  The
// result is ONE device batch.  Throws ChqError; DESIGN.md section 3.8.
Batch join_records(Context& ctx, std::vector<Batch>& left, const chq_table_aliases* left_aliases, std::vector<Batch>& right,
                   const chq_table_aliases* right_aliases, const std::vector<JoinKeyArg>& keys, int kind = CHQ_JOIN_INNER);

}  // namespace chq
