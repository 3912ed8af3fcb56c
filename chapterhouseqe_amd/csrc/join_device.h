// join_device.h -- parameter blocks of the INNER JOIN kernels (join.hip), shared with the host side (join.cpp).
//
// The join runs on top of the stable sort and the group heads of GROUP BY: the keys of both sides are concatenated, RIGHT
// rows first (row ids [0, nR)), then LEFT rows (row ids [nR, nR + nL)), and sorted; a run of equal keys is then laid out as
// [its right rows in input order][its left rows in input order].  `gids` / `starts` come from the agg_head_* kernels.
// Data passes between workgroups only at launch boundaries.  DESIGN.md section 3.8.
#pragma once
#include <stdint.h>

#include "aggregate_device.h"

namespace chq {

constexpr int kJoinBlock = kAggBlock;   // threads of every join kernel's workgroup (4 waves)
constexpr int kJoinItems = kAggItems;   // sorted positions, left rows or output rows per thread
constexpr int kJoinTile = kAggTile;     // ... per workgroup tile

struct JoinSplitParams {   // join_split_kernel: split[g] = the sorted position where the left rows of group g begin
  const uint32_t* perm;      // [n] (null: identity)
  int64_t n;                 // nR + nL
  int64_t n_right;
  const uint32_t* gids;      // [n]
  const uint32_t* starts;    // [G + 1]
  uint32_t* split;           // [G]
  // a group in which one of these keys is null matches nothing: split[g] = starts[g] (no right rows)
  const uint8_t* validity[kAggMaxKeys];   // null: the key has no nulls
  int64_t bit_offset[kAggMaxKeys];
  int32_t n_keys;
  int32_t nulls_only;        // a later launch of the same call (more than kAggMaxKeys keys): only the null rule is applied
};

struct JoinCountParams {   // join_count_kernel: for the position of left row l: cnt[l] = matching right rows, first[l] = their first position
  const uint32_t* perm;      // [n] (null: identity)
  int64_t n;
  int64_t n_right;
  const uint32_t* gids;      // [n]
  const uint32_t* starts;    // [G + 1]
  const uint32_t* split;     // [G]
  uint32_t* cnt;             // [nL]
  uint32_t* first;           // [nL]
};

struct JoinScanParams {   // join_tile_sums_kernel, join_scan_sums_kernel (one workgroup), join_offsets_kernel
  const uint32_t* cnt;       // [nL]
  int64_t n_left;
  int64_t ntiles;            // tiles of kJoinTile left rows
  uint64_t* tile_sums;       // [ntiles + 1]: matches per tile; after the scan their exclusive prefix, then the total M
  uint32_t* off;             // [nL]: output rows before left row l (exact once M < 2^32 is known)
};

struct JoinExpandParams {   // join_expand_kernel: output j -> (left row, right row)
  const uint32_t* perm;      // [n] (null: identity)
  const uint32_t* off;       // [nL]
  const uint32_t* first;     // [nL]
  int64_t n_left;
  int64_t m;                 // output rows
  uint32_t* lidx;            // [m] left row of output j: the largest l with off[l] <= j
  uint32_t* ridx;            // [m] right row of output j: perm[first[l] + (j - off[l])]
};

}  // namespace chq
