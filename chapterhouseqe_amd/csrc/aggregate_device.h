// aggregate_device.h -- parameter blocks of the GROUP BY kernels (aggregate.hip), shared with the host side (aggregate.cpp).
//
// GROUP BY runs on top of the stable sort: `perm` orders the rows by the keys (ascending, nulls last), so every group is one
// run of consecutive SORTED POSITIONS.  The kernels find the first position of every run (group heads), number the runs (head
// scan) and reduce every aggregate over its runs (segmented reduce + fold).  Data passes between workgroups only at launch
// boundaries.  DESIGN.md section 3.7.
#pragma once
#include <stdint.h>

namespace chq {

constexpr int kAggBlock = 256;                    // threads of every aggregate kernel's workgroup (4 waves)
constexpr int kAggItems = 8;                      // consecutive sorted positions per thread
constexpr int kAggTile = kAggBlock * kAggItems;   // sorted positions per workgroup tile
constexpr int kAggMaxKeys = 8;                    // keys compared by one group-heads launch (more keys: more launches)

// how the heads kernel compares the values of one key
enum AggKeyKind : int32_t {
  AK_FIXED = 0,   // `width` bytes (1, 2, 4, 8, 16), compared as bits
  AK_BOOL,        // bit of a bitmap
  AK_UTF8,        // int32 offsets + bytes: equal length, then equal bytes
};

struct AggKey {
  const uint8_t* values;     // fixed width: values of row 0; Boolean: bitmap; Utf8: int32 offsets of row 0
  const uint8_t* data;       // Utf8 bytes (offsets are absolute into it; null: every string is empty)
  const uint8_t* validity;   // null: no nulls
  int64_t bit_offset;        // bit position of row 0 in `validity` and in a Boolean bitmap
  int32_t kind;              // AggKeyKind
  int32_t width;             // AK_FIXED
};

struct AggHeadsParams {   // agg_heads_kernel: heads[i] = i == 0 || some key differs between rows perm[i-1] and perm[i]
  const uint32_t* perm;      // null: identity
  int64_t n;
  uint8_t* heads;            // [ntiles * kAggTile] (positions >= n: 0)
  uint32_t* tile_counts;     // [ntiles + 1]: heads per tile; after agg_head_scan_kernel their exclusive scan, then G
  int64_t ntiles;
  AggKey keys[kAggMaxKeys];
  int32_t n_keys;
  int32_t accumulate;        // a later launch of the same call: heads |= ...
};

struct AggGroupsParams {   // agg_head_scan_kernel (one workgroup), then agg_head_write_kernel (one workgroup per tile)
  const uint32_t* perm;      // null: identity
  int64_t n;
  const uint8_t* heads;
  uint32_t* tile_counts;     // [ntiles + 1]
  int64_t ntiles;
  uint32_t* gids;            // [n]: group of every sorted position
  uint32_t* starts;          // [G + 1]: first sorted position of every group; starts[G] = n
  uint32_t* rep;             // [G]: the group's first row in input order, perm[starts[g]]
  int64_t G;                 // write kernel only (read back after the scan)
};

// AO_AVG_INT / AO_AVG_FLOAT accumulate exactly like AO_SUM_INT / AO_SUM_FLOAT -- the same identity, load, combine and tree --
// and differ only in the value written for a finished group: the total over the count (aggregate_acc.h: acc_finalize)
enum AggOp : int32_t { AO_COUNT = 0, AO_SUM_INT, AO_SUM_FLOAT, AO_MIN, AO_MAX, AO_AVG_INT, AO_AVG_FLOAT };
// how a value is read (AO_SUM_INT: widened to 128 bits; AO_MIN / AO_MAX: mapped to an order-preserving u64 and back)
enum AggValueKind : int32_t { AV_SIGNED = 0, AV_UNSIGNED, AV_FLOAT };

// One accumulator shape for every aggregate: cnt = non-null values; a (, b) by AggOp:
//   AO_SUM_INT    a = low, b = high word of the exact 128-bit total (AO_AVG_INT too)
//   AO_SUM_FLOAT  a = bits of the binary64 partial sum (AO_AVG_FLOAT too)
//   AO_MIN/AO_MAX a = order-preserving u64 of the value (sort.hip: sort_norm_kernel)
struct AggAcc {
  uint64_t a, b, cnt;
};

struct AggReduceParams {   // agg_reduce_kernel (one workgroup per tile), then agg_fold_kernel (one per tile boundary)
  const uint32_t* perm;      // null: identity
  int64_t n;
  int64_t ntiles;
  const uint32_t* gids;      // [n]
  const uint32_t* starts;    // [G + 1]
  int64_t G;
  const uint8_t* values;     // values of row 0 (null: AO_COUNT)
  const uint8_t* validity;   // null: no nulls
  int64_t bit_offset;
  AggAcc* part_first;        // [ntiles]: the tile's share of a group that began in an earlier tile
  AggAcc* part_last;         // [ntiles]: the tile's share of a group that begins in it and goes on behind it
  uint8_t* out;              // [G] values: i64 (AO_COUNT), 8 bytes (sums, averages), `width` bytes (AO_MIN / AO_MAX)
  uint64_t* cnt_out;         // [G] non-null values per group (null: AO_COUNT)
  uint32_t* overflow;        // AO_SUM_INT: set when a group's exact total does not fit 64 bits (AO_AVG_INT never touches it)
  int32_t op;                // AggOp
  int32_t value_kind;        // AggValueKind
  int32_t width;             // bytes per input value
  int32_t pad;
};

struct AggCountStarParams {   // agg_count_star_kernel: out[g] = starts[g + 1] - starts[g]
  const uint32_t* starts;
  int64_t G;
  int64_t* out;
};

// agg_distinct_kernel: COUNT(DISTINCT c).  The rows sorted by (keys, c) have the FINE runs starts2 / rep2 (runs of equal keys
// and equal c); group g covers the same sorted positions [starts[g], starts[g + 1]) under that order as under the keys' own,
// and the null values of c are the last fine run inside it.  out[g] = fine runs inside the group, less the null run.
struct AggDistinctParams {
  const uint32_t* starts;    // [G + 1]
  int64_t G;
  const uint32_t* starts2;   // [G2 + 1], ascending, starts2[G2] = n; every starts[g] is among them
  const uint32_t* rep2;      // [G2]: one row of every fine run
  int64_t G2;
  const uint8_t* validity;   // of c (null: no nulls)
  int64_t bit_offset;
  int64_t* out;              // [G]
};

struct AggValidityParams {   // agg_validity_kernel: bit g = cnt[g] != 0; *ones += set bits
  const uint64_t* cnt;
  int64_t G;
  uint8_t* out;              // bitmap, u32 words
  uint64_t* ones;            // zeroed by the caller
};

}  // namespace chq
