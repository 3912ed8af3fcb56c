// sort_device.h -- parameter blocks of the ORDER BY kernels (sort.hip), shared with the host side (sort.cpp).
//
// Kept apart from device_program.h: that header rebuilds the four kernels.hip units.
//
// The sort works on (u64 key word, u32 row id) pairs.  A sort key is lowered into one or more key words whose
// unsigned order is the wanted order (sort.cpp: key_words); the words are radix-sorted least significant first, each
// one a stable LSD radix sort of 8-bit digits, so the permutation after the last word is the stable lexicographic
// order of every key.
#pragma once
#include <stdint.h>

namespace chq {

constexpr int kSortBlock = 256;                      // threads of every sort kernel's workgroup (4 waves)
constexpr int kSortItems = 8;                        // pairs per thread in a radix pass
constexpr int kSortTile = kSortBlock * kSortItems;   // pairs per workgroup tile (count / scatter / Utf8 offsets)

// how a key word is built from a column value
enum SortWordKind : int32_t {
  SW_SIGNED = 0,    // two's complement integer of `width` bytes: sign-extended, sign bit flipped
  SW_UNSIGNED,      // unsigned integer of `width` bytes
  SW_FLOAT,         // IEEE float of `width` bytes: totalOrder flip (sign set: all bits inverted, else sign bit set)
  SW_BOOL,          // bit of a bitmap (false < true)
  SW_DEC_LO,        // Decimal128: low 64 bits, unsigned
  SW_DEC_HI,        // Decimal128: high 64 bits, signed
  SW_UTF8_LEN,      // Utf8: byte length (the tie-break of equal zero-padded bytes: a proper prefix sorts first)
  SW_UTF8_CHUNK,    // Utf8: bytes [8 chunk, 8 chunk + 8) big-endian, zero-padded
  SW_NULL_FLAG,     // 0 / 1 by validity: nulls before (nulls_first) or after the non-null rows
};

struct SortNormParams {   // sort_norm_kernel: keys[i] = word(row perm[i]), vals[i] = perm[i]
  const uint32_t* perm;        // null: identity
  uint64_t* keys;
  uint32_t* vals;
  int64_t n;
  const uint8_t* values;       // fixed width: values of row 0; Boolean: bitmap; Utf8: int32 offsets of row 0
  const uint8_t* data;         // Utf8 bytes (offsets are absolute into it)
  const uint8_t* validity;     // null: no nulls
  int64_t bit_offset;          // bit position of row 0 in `validity` and in a Boolean bitmap
  int64_t chunk;               // SW_UTF8_CHUNK
  uint64_t invert;             // xor applied to a non-null row's word (all ones: descending)
  int32_t kind;                // SortWordKind
  int32_t width;               // bytes per value (fixed width kinds)
  int32_t nulls_first;         // SW_NULL_FLAG
  int32_t pad;
};

struct SortHistParams {   // sort_hist_kernel: hist[b][d] = keys whose byte b is d, every byte in one read
  const uint64_t* keys;
  int64_t n;
  uint32_t* hist;              // [8][256], zeroed by the caller
};

struct SortPassParams {   // one 8-bit digit pass: count -> scan -> scatter
  const uint64_t* keys_in;
  const uint32_t* vals_in;
  uint64_t* keys_out;
  uint32_t* vals_out;
  int64_t n;
  int64_t ntiles;              // ceil(n / kSortTile)
  uint32_t* tile_counts;       // [256][ntiles]: counts, then (scan) first output position of (digit, tile)
  const uint32_t* digit_hist;  // [256]: keys per digit of this pass (from sort_hist_kernel)
  int32_t shift;               // bit position of the digit
  int32_t pad;
};

struct SortMaxLenParams {   // sort_utf8_maxlen_kernel: *out = max byte length of rows [0, n)
  const int32_t* offsets;      // offsets of row 0
  int64_t n;
  uint32_t* out;               // zeroed by the caller
};

constexpr uint32_t kSortNoRow = 0xFFFFFFFFu;   // "no row" in a row-id list (the padded variants of the gathers; never a row: a call takes fewer than 2^32 - 1)

struct SortGatherParams {   // the final permutation applied to one column: out row i = in row perm[i]
  const uint32_t* perm;        // padded variants: an entry may be kSortNoRow, and the output row is then null
  int64_t m;                   // output rows
  const uint8_t* in;           // fixed width: values of row 0; bits: bitmap; Utf8: int32 offsets of row 0
  int64_t in_bit_offset;       // bits: position of row 0
  uint8_t* out;                // fixed width: values; bits: bitmap (u32 words); Utf8: int32 offsets [m + 1]
  const uint8_t* in_data;      // Utf8: bytes
  uint8_t* out_data;           // Utf8: bytes
  uint64_t* tile_sums;         // Utf8: [ceil(m / kSortTile) + 1] byte totals, then their exclusive scan (+ the grand total)
  int64_t ntiles;
  uint64_t* ones;              // bits: count of set output bits (null_count = m - ones), zeroed by the caller
  int32_t width;               // fixed width: 1, 2, 4, 8, 16
  int32_t pad;
};

}  // namespace chq
