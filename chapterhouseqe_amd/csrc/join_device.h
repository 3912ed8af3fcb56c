// join_device.h -- parameter blocks of the join kernels (join.hip), shared with the host side (join.cpp): INNER, and the
// LEFT / FULL / LEFT_SEMI / LEFT_ANTI kinds on top of it (RIGHT is LEFT with the sides exchanged on the host).
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
constexpr uint32_t kJoinNoRow = 0xFFFFFFFFu;   // "no row" in a row-id list (= kSortNoRow of the gathers) and in first[]: both
                                               // sides together hold fewer than 2^32 rows, so ids and positions stop at 2^32 - 2

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

// how many output rows a left row with c matching right rows gives (join_count_kind_kernel)
enum JoinCountRule : int32_t {
  JOIN_COUNT_PADDED = 1,   // LEFT, FULL: max(c, 1) -- an unmatched row gives one padded row, marked by first[l] = kJoinNoRow
  JOIN_COUNT_SEMI = 2,     // c > 0
  JOIN_COUNT_ANTI = 3,     // c == 0
};

struct JoinCountKindParams {   // join_count_kind_kernel: join_count_kernel with a count rule
  JoinCountParams base;
  int32_t rule;              // JoinCountRule
  int32_t pad;
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
// join_expand_kind_kernel takes the same block: with right rows, first[l] == kJoinNoRow gives ridx[j] = kJoinNoRow; without
// (SEMI, ANTI: every count is 0 or 1), ridx and first are not touched and may be null.

struct JoinTailParams {   // FULL's tail: the right rows no left row matches, ascending, behind the LEFT rows
  const uint32_t* perm;      // [n] (null: identity)
  int64_t n;
  int64_t n_right;
  const uint32_t* gids;      // [n]
  const uint32_t* starts;    // [G + 1] (starts[G] = n)
  const uint32_t* split;     // [G]
  uint32_t* flag;            // [nR] join_tail_flag_kernel: 1 iff right row r is in a run with a null key or without left rows
  const uint32_t* off;       // [nR] join_tail_write_kernel: exclusive scan of flag (launch_offsets_scan)
  int64_t m_left;            // rows of the LEFT part
  int64_t m;                 // m_left + the tail's length
  uint32_t* lidx;            // [m] lidx[m_left + off[r]] = kJoinNoRow
  uint32_t* ridx;            // [m] ridx[m_left + off[r]] = r
};

}  // namespace chq
