// typed_ops.h -- parameter blocks of the small kernels of typed_ops.hip and scan.hip that are not part of the device program
// interface (device_program.h, whose hash ties the committed PMC summaries to the kernels they were measured on).
#pragma once
#include <stdint.h>

namespace chq {
// The launch grid of typed_ops.hip, like.hip, strfn.hip, case.hip and cast.hip: one thread per item in workgroups of 256
// (wave_rows.h: kRowsBlock), at least one workgroup and at most cap_blocks; the kernels walk what is left in rounds.
inline unsigned rows_grid(int64_t items, int64_t cap_blocks) {
  const int64_t blocks = (items + 255) / 256;
  return (unsigned)(blocks < 1 ? 1 : blocks > cap_blocks ? cap_blocks : blocks);
}

// Uniform-length Utf8 columns (keys, hashes, the reference's sample strings): utf8_uniform_kernel checks that every value
// of a column has the length of the first one; out = {1 if some value differs, that length, offsets[0]}.
// iota_offsets_kernel writes the offsets of n values of L bytes: 0, L, 2 L, ...
struct Utf8UniformParams { const int32_t* offsets; int64_t nrows; int32_t* out; };
struct IotaOffsetsParams { int32_t* out; int64_t n_plus_1; int32_t step; int32_t pad; };
// the same check for every batch of a group: block b walks batch b's offsets; out[3 b ..] = {differs, length, offsets[0]}
struct Utf8UniformGroupParams { const unsigned long long* offsets_of; const long long* rows_of; int64_t nb; int32_t* out; };
// IS [NOT] NULL: is_null_kernel re-aligns a validity bitmap read from bit `validity_offset` to bit 0 of `out_bits`
// ((nrows + 63) / 64 words), complemented for IS NULL (`negated` = 0); without a bitmap every row is valid.
struct IsNullParams { const void* validity; int64_t validity_offset; int64_t nrows; unsigned long long* out_bits; int32_t negated; int32_t pad; };
// scan.hip, launch_offsets_scan: out[i] = len[0] + ... + len[i - 1] (mod 2^32) for i in [0, n), in three launches -- the
// 64-bit sum of every tile of 2048 lengths (the callers' kJoinTile, STRFN_SCAN_CHUNK), the exclusive scan of the sums by one
// workgroup, which leaves the 64-bit total in tile_sums[ntiles], and the offsets of every tile.  The lengths are read as
// UNSIGNED.  The caller reads the total back and refuses what 32 bits cannot hold before anything reads offsets that wrapped.
struct OffsetsScanParams {
  const uint32_t* len;       // [n]
  int64_t n;
  int64_t ntiles;            // ceil(n / 2048)
  uint64_t* tile_sums;       // [ntiles + 1]
  uint32_t* out;             // [n], or [n + 1] with write_total
  int32_t write_total;       // out[n] = the total, truncated to 32 bits (Arrow offsets)
  int32_t pad;
};
}  // namespace chq
