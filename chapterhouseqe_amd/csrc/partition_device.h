// partition_device.h -- parameter blocks of the hash partitioning kernels (partition.hip), shared with the host side
// (partition.cpp).
//
// A partitioning is ONE radix pass of the sort (sort.hip) whose "digit" is the partition id of a row: hash + count -> scan ->
// scatter, three launches that hand data over only at launch boundaries.  Only the ids (1 byte per row) and the permutation
// (4 bytes per row) move; the keys are hashed in place.  DESIGN.md section 3.9.
#pragma once
#include <stdint.h>

namespace chq {

constexpr int kPartBlock = 256;                       // threads of every partition kernel's workgroup (4 waves)
constexpr int kPartItems = 8;                         // rows per thread
constexpr int kPartTile = kPartBlock * kPartItems;    // rows per workgroup tile
constexpr int kPartMaxKeys = 8;                       // keys hashed by one launch (more keys: more launches)
constexpr int kPartMaxPartitions = 256;               // a partition id is one byte; one thread per partition in a workgroup

// how the hash kernel reads the values of one key
enum PartKeyKind : int32_t {
  PK_FIXED = 0,   // `width` bytes (1, 2, 4, 8, 16): one chunk (16: two, low word first)
  PK_BOOL,        // bit of a bitmap: one byte holding 0 or 1
  PK_UTF8,        // int32 offsets + bytes: 8-byte chunks, the last one zero-padded
};

struct PartKey {
  const uint8_t* values;     // fixed width: values of row 0; Boolean: bitmap; Utf8: int32 offsets of row 0
  const uint8_t* data;       // Utf8 bytes (offsets are absolute into it; null: every string is empty)
  const uint8_t* validity;   // null: no nulls
  int64_t bit_offset;        // bit position of row 0 in `validity` and in a Boolean bitmap
  int32_t kind;              // PartKeyKind
  int32_t width;             // PK_FIXED
};

struct PartHashParams {   // part_hash_kernel: the row hash over `keys`; the last launch of a call writes ids and counts
  int64_t n;
  int64_t ntiles;            // ceil(n / kPartTile)
  PartKey keys[kPartMaxKeys];
  int32_t n_keys;
  int32_t first;             // the first launch of the call: h starts from the seed, else from carry[row]
  int32_t last;              // the last launch of the call: ids, tile_counts and totals are written, else carry[row] = h
  uint32_t n_partitions;     // [1, kPartMaxPartitions]
  uint64_t* carry;           // [n] (more than kPartMaxKeys keys)
  uint8_t* ids;              // [n]
  uint32_t* tile_counts;     // [n_partitions][ntiles]: rows of (partition, tile)
  uint32_t* totals;          // [n_partitions]: rows per partition, zeroed by the caller
};

struct PartScatterParams {   // part_scan_kernel (one workgroup per partition), then part_scatter_kernel (one per tile)
  int64_t n;
  int64_t ntiles;
  const uint8_t* ids;        // [n]
  uint32_t* tile_counts;     // [n_partitions][ntiles]: counts, then (scan) first output position of (partition, tile)
  const uint32_t* totals;    // [n_partitions]
  uint32_t n_partitions;
  uint32_t pad;
  uint32_t* perm;            // [n]: the rows of partition 0 in input order, then those of partition 1, ...
};

}  // namespace chq
