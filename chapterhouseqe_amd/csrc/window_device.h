// window_device.h -- parameter blocks of the window-function kernels (window.hip), shared with the host side (window.cpp).
//
// A window call runs on top of the stable sort and of GROUP BY's run finder: `perm` orders the rows by the partition keys,
// then the order keys, so a partition is one run of consecutive SORTED POSITIONS (pgid / pstarts) and a peer group a run
// inside it (qgid / qstarts).  Every kernel works on sorted positions and writes its result to the row's place in INPUT
// order, out[perm[i]].  Data passes between workgroups only at launch boundaries.  DESIGN.md section 3.10.
#pragma once
#include <stdint.h>

#include "aggregate_device.h"

namespace chq {

constexpr int kWinBlock = kAggBlock;        // threads of every window kernel's workgroup (4 waves)
constexpr int kWinItems = kAggItems;        // sorted positions per thread
constexpr int kWinTile = kAggTile;          // sorted positions per workgroup tile
constexpr int kWinCarryRound = kWinBlock;   // tiles one round of win_carry_kernel covers (one per thread)

enum WinFrame : int32_t {   // = chq_window_frame
  WF_PARTITION = 0,         // the whole partition
  WF_ROWS = 1,              // the partition's first row .. this row
  WF_RANGE = 2,             // the partition's first row .. this row's last peer
};

struct WinRankParams {   // win_rank_kernel: every ranking item of a call (an output that is not asked for: null)
  const uint32_t* perm;      // null: identity
  int64_t n;
  const uint32_t* pgid;      // [n]: partition of every sorted position
  const uint32_t* pstarts;   // [P + 1]
  const uint32_t* qgid;      // [n]: peer group of every sorted position (null: neither rank nor dense_rank)
  const uint32_t* qstarts;   // [Q + 1]
  int64_t* row_number;       // [n], input order
  int64_t* rank;
  int64_t* dense_rank;
};

struct WinShiftParams {   // win_shift_kernel: src[perm[i]] = perm[i + delta] inside the partition of i, else kSortNoRow
  const uint32_t* perm;      // null: identity
  int64_t n;
  const uint32_t* pgid;
  const uint32_t* pstarts;
  int64_t delta;             // LAG: -offset, LEAD: +offset (|delta| <= 2^32)
  uint32_t* src;             // [n], input order: the row list of the null-producing gather
};

// The segmented inclusive scan of one aggregate over the partitions, and what reads it: win_scan_kernel (one workgroup per
// tile), win_carry_kernel (one workgroup), win_emit_kernel (one workgroup per tile).  The scanned element is GROUP BY's
// accumulator (AggAcc), kept as one array per word so that an aggregate stores only the words it has.
struct WinAggParams {
  const uint32_t* perm;      // null: identity
  int64_t n;
  int64_t ntiles;
  const uint32_t* pgid;
  const uint32_t* pstarts;
  const uint32_t* qgid;      // WF_RANGE only
  const uint32_t* qstarts;
  const uint8_t* values;     // values of row 0 (null: AO_COUNT)
  const uint8_t* validity;   // null: no nulls
  int64_t bit_offset;
  uint64_t* scan_a;          // [n] AggAcc::a of the tile-local scan (not AO_COUNT)
  uint64_t* scan_b;          // [n] AggAcc::b (AO_SUM_INT only)
  uint32_t* scan_cnt;        // [n] AggAcc::cnt.  Null in win_emit_kernel: no scan ran, the count is the frame's rows
  AggAcc* tile_tot;          // [ntiles]: the tile-local scan at the tile's last position (its open run)
  AggAcc* tile_carry;        // [ntiles]: the segmented inclusive scan of tile_tot
  uint8_t* out;              // [n] values in input order: i64 (AO_COUNT), 8 bytes (sums), `width` bytes (AO_MIN / AO_MAX)
  uint64_t* cnt_out;         // [n] non-null values of the row's frame, input order (null: AO_COUNT)
  uint32_t* overflow;        // AO_SUM_INT: set when the exact total of some row's frame does not fit 64 bits
  int32_t op;                // AggOp
  int32_t value_kind;        // AggValueKind
  int32_t width;             // bytes per input value
  int32_t frame;             // WinFrame
};

}  // namespace chq
