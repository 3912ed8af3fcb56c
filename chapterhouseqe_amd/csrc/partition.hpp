// partition.hpp -- hash partitioning of a group of record batches by key columns (partition.cpp): the primitive that lets a
// keyed operator (join.hpp, aggregate.hpp) run on more than one instance, on top of the gathers of the sort (sort.hpp).
#pragma once
#include <cstdint>
#include <vector>

#include "sort.hpp"
#include "partition_device.h"

namespace chq {

// partition.hip
hipError_t launch_part_hash(const PartHashParams& p, hipStream_t stream);
hipError_t launch_part_scatter(const PartScatterParams& p, hipStream_t stream);   // scan, scatter: 2 launches

// The rows of `in` (one schema, host or device resident) cut into `n_partitions` parts by the pinned hash of the key columns
// `keys` (include/chq.h: chq_partition_records): ONE device batch holding the rows of part 0 in input order (batch order,
// then row order), then those of part 1, ...; ends[p] = the exclusive end row of part p.  Throws ChqError; DESIGN.md
// section 3.9.
JoinedGroup partition_records(Context& ctx, std::vector<Batch>& in, const chq_table_aliases* aliases, const std::vector<const Expr*>& keys,
                              int n_partitions);

}  // namespace chq
