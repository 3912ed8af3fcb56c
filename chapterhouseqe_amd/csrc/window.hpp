// window.hpp -- window functions: ROW_NUMBER / RANK / DENSE_RANK, LAG / LEAD and framed COUNT / SUM / MIN / MAX over
// (PARTITION BY ... ORDER BY ...) of a record batch, or of a group of them joined into one (window.cpp), on top of the
// stable sort (sort.hpp) and GROUP BY's run finder (aggregate.hpp).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "aggregate.hpp"
#include "window_device.h"

namespace chq {

// window.hip
hipError_t launch_win_rank(const WinRankParams& p, hipStream_t stream);
hipError_t launch_win_shift(const WinShiftParams& p, hipStream_t stream);
hipError_t launch_win_scan(const WinAggParams& p, hipStream_t stream);   // scan, then carry: 2 launches
hipError_t launch_win_emit(const WinAggParams& p, hipStream_t stream);

// one output column as the C ABI hands it over (chq_window_item)
struct WinItemArg {
  int kind = 0;                   // chq_window_kind
  int frame = 0;                  // chq_window_frame (the aggregates)
  int64_t offset = 0;             // LAG / LEAD
  const Expr* column = nullptr;   // LAG / LEAD and the aggregates but COUNT(*): Identifier / CompoundIdentifier
  std::string name;               // output column name
};

// Every row of the batches of `in` (one schema, host or device resident) IN INPUT ORDER: the input columns, then one
// column per item.  The result is ONE device batch.  Throws ChqError; DESIGN.md section 3.10.
Batch window_records(Context& ctx, std::vector<Batch>& in, const chq_table_aliases* aliases, const std::vector<const Expr*>& partition_by,
                     const std::vector<SortKeyArg>& order_by, const std::vector<WinItemArg>& items);

}  // namespace chq
