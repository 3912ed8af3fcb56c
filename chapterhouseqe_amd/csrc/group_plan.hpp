// group_plan.hpp -- the batch-group filter's host plans (group_plan.cpp): the flat description of a group's batches, eligibility,
// tiling, the layout of the group table and its writer, the size rules of the folded Utf8 columns, the chunk cuts and the word
// layout of the concat tables.  Plain values, no Context, no HIP: tests/group_plan_main.cpp runs the unit on the CPU.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "plan.hpp"   // DType, u64, MAX_OUT, MAX_FOLD_UTF8 (device_program.h)

struct ArrowDeviceArray;
struct ArrowSchema;

namespace chq {
struct Batch;

// cleared bits among bits [offset, offset + n) of a host bitmap (inline: the per-call host paths use it).  It lives here,
// not in engine.hpp, because put_column counts an uncounted host bitmap with it and this header must stand without the engine.
inline int64_t count_nulls_host(const uint8_t* validity, int64_t offset, int64_t n) {
  int64_t nulls = 0;
  for (int64_t i = 0; i < n; ++i) { int64_t b = offset + i; nulls += !((validity[b >> 3] >> (b & 7)) & 1); }
  return nulls;
}

// rows of a tile, of one wave's share of it, and waves per tile, by tile kind (the filter kernel's three instantiations).
// kTileRows came over from engine_internal.hpp for the same reason: the tiling is planned here, and the engine reads it from here.
constexpr int64_t kTileRows[3] = {1024 * 16, 256 * 8, 256 * 8};
constexpr int64_t kWaveRows[3] = {64 * 16, 64 * 8, 64 * 8};
constexpr int64_t kWavesPerTile[3] = {16, 4, 4};

struct GroupCol { DType type; int64_t width; };   // the schema as the plans see it
struct GroupOptions {                             // Context::opt_* of the same names
  int64_t tile_kind = -1, group_mode = 0, group_bits = 1, fold_utf8 = 1, group_fold = 1, group_chunk_bytes = 1ll << 30;
};

// Per-batch facts of a group in flat arrays, gathered while the batches are imported (capi.cpp: the Arrow structs of 10^4
// batches are ~10^5 dependent cache misses, taken once, on the pool's threads).  Later passes of a group call -- eligibility,
// row totals, pointer tables -- read these arrays instead of walking the Batch objects again.
struct GroupLite {
  size_t ncols = 0;
  std::vector<int64_t> rows;               // [nb]
  std::vector<const uint8_t*> values0;     // [nb * ncols] Column::values0() (Boolean: the bitmap)
  std::vector<const uint8_t*> data;        // [nb * ncols] Utf8 bytes
  std::vector<const uint8_t*> validity;    // [nb * ncols] validity bitmap, null when the column has no nulls in that batch
  std::vector<int64_t> offset;             // [nb * ncols] Arrow slice offset: bit position of row 0 in the bitmaps
  std::vector<uint8_t> flags;              // [nb] GL_*
  // GL_NULLS: a validity bitmap that may clear a bit (device batch: bitmap present and null_count != 0; host batch: nulls
  // counted, by the producer or here).  GL_ON_DEVICE: in this context's GPU memory.  GL_ON_HOST: in host memory.
  enum : uint8_t { GL_NULLS = 1, GL_NO_UTF8_DATA = 2, GL_SCHEMA_DIFFERS = 4, GL_ON_DEVICE = 8, GL_SHORT = 16, GL_ON_HOST = 32 };
  void resize(size_t nb, size_t nc) { ncols = nc; rows.assign(nb, 0); values0.assign(nb * nc, nullptr); data.assign(nb * nc, nullptr); validity.assign(nb * nc, nullptr); offset.assign(nb * nc, 0); flags.assign(nb, 0); }
  // the facts of batch b from an imported batch / straight from the Arrow structs of a device batch (no Batch object): arrow_io.cpp
  void set(size_t b, const Batch& r, const Batch& first, int device);
  void set_from_arrow(size_t b, const ArrowDeviceArray* rec, const ArrowSchema* schema, const Batch& first, int device);
  // One column (type and width of `kind`) of one batch into slot `at`; returns the GL_* bits it contributes.  What both
  // setters must agree on: values0 with the slice offset applied (Boolean: the bitmap itself), the Utf8 bytes, the bit
  // offset, and the validity bitmap only where it may clear a bit.
  uint8_t put_column(size_t at, GroupCol kind, bool on_host, const uint8_t* bitmap, int64_t null_count, int64_t length,
                     const uint8_t* values, const uint8_t* bytes, int64_t off);
  GroupLite slice(size_t b0, size_t b1) const;   // the facts of batches [b0, b1)
};

// ---- eligibility: one scan of the per-batch flags ------------------------------------------------------------------------
struct GroupPlan {
  bool per_batch = false;    // a batch of fewer than 2 rows, or another schema: the per-batch loop
  bool plain = false;        // fixed-width columns without nulls (wave-packed device groups: bitmaps too): the one-launch path
  bool fold = false;         // device-resident short-string Utf8 columns (`fold_utf8`): filtered straight out of the batches
  bool need_bits = false;    // validity bitmaps / Boolean columns ride along (compacted behind the main kernel)
  bool host_in = false, all_host = false;
  bool all_device = false;   // every batch in this GPU's memory
  bool resident = false;     // every batch where batch 0 is (host memory, or this GPU's)
  int64_t total_rows = 0, max_rows = 0;
  std::vector<int> fold_utf8;
};
// `host_in`: batch 0 lies in host memory
GroupPlan plan_group(const std::vector<uint8_t>& flags, const std::vector<int64_t>& rows, const std::vector<GroupCol>& schema,
                     bool host_in, const GroupOptions& opt);

// ---- tiling ----------------------------------------------------------------------------------------------------------------
// wpb > 0: wave-packed (every batch owns wpb consecutive waves); wpb == 0: whole tiles per batch, one table row per tile
struct GroupTiling { int tile_kind = 0; int64_t wpb = 0, ntiles = 0; };
GroupTiling plan_tiling(bool wide_or_temps, const GroupOptions& opt, const std::vector<int64_t>& rows, int64_t total_rows, int64_t max_rows);

// ---- the group table ---------------------------------------------------------------------------------------------------------
// The contract with filter_fused_kernel and bit_compact_group_kernel (FilterParams::group, BitCompactGroupParams::table).
// One block of 64-bit words: the table, then the index of every batch's last tile (tile mode only), then the per-batch
// end offsets the launch writes.  The table has one row of `stride` words per BATCH (wave mode) or per TILE (tile mode;
// tiles never straddle batches and a batch's tiles are consecutive).  A row, in order:
//
//   wave mode   [0]           rows of the batch
//   tile mode   [0] [1]       first row of the tile inside its batch, rows of the batch
//   then        n_refs        value pointer of every program column-ref (Lowered::refs), at row 0 of the batch
//               n_out         input pointer of every copied column, in launch order (the stashed column last)
//               2 x n_fold    per folded Utf8 column: its int32 offsets at row 0, its bytes
//   bits_at:    n_refs        bitmap of every program column-ref (its validity; 0: every row valid)       } only with
//               n_refs        bit position of the batch's row 0 in that bitmap                            } need_bits,
//               2 x n_bits    per bit column (BitCol::word): {bitmap, bit position of row 0} -- column by } wave mode
//                             column, a Boolean column's values, then its validity if any batch has nulls in it
//
// bits_at = 0 says "no bitmaps" (word 0 is always taken).  Declined (ok = false): bitmaps on a group that is not wave-packed,
// more than 16 bit columns (one null counter each in the scratch header), folded Utf8 columns under tile kind 2.
struct BitCol { int col; bool validity; size_t word; };   // word: index of {bitmap, bit offset} in a batch's table row
struct GroupTableLayout {
  bool ok = false;
  size_t stride = 0, bits_at = 0;
  size_t table_rows = 0;                          // nb (wave mode) or ntiles
  size_t bytes_tbl = 0, bytes_idx = 0, bytes_cnt = 0;
};
GroupTableLayout layout_group_table(const GroupTiling& tl, size_t nb, size_t n_refs, size_t n_out, size_t n_fold, bool need_bits,
                                    std::vector<BitCol>& bit_cols);
// The table and (tile mode) the last-tile index into `block` (bytes_tbl + bytes_idx bytes of it), in one pass over the flat
// arrays.  `in_ptr`: [batch][column] value pointers as the device sees them (lite.values0, or where a host group was staged).
void write_group_table(const GroupTableLayout& lay, const GroupTiling& tl, const GroupLite& lite, const uint8_t* const* in_ptr,
                       const std::vector<int>& refs, const std::vector<int>& outs, const std::vector<int>& fold,
                       const std::vector<BitCol>& bit_cols, u64* block);

// ---- folded Utf8 columns: do the joined strings fit ONE output column? --------------------------------------------------------
// `bytes[k][b]`: data bytes of the k-th folded column of batch b.  `cap`: bytes per column.  `short_strings`: at most 24 bytes
// a row on average in every column; `fits`: short, and below what int32 offsets address -- 2 x group_chunk_bytes - 64 = 2 GiB
// unless a test lowers the option.
struct FoldSizes { bool fits = true, short_strings = true; std::vector<int64_t> cap; };
FoldSizes fold_sizes(const std::vector<std::vector<int64_t>>& bytes, int64_t total_rows, int64_t chunk_bytes);

// Chunks [cuts[k], cuts[k+1]) of a group: a cut before the batch at which the rows would pass 2^30 or the bytes of any Utf8
// column would pass `limit` (int32 offsets of the joined output; a batch over the limit on its own is a chunk of its own).
// `bytes[k][b]`: data bytes of the k-th Utf8 column of batch b.
std::vector<size_t> chunk_cuts(const std::vector<int64_t>& rows, const std::vector<std::vector<int64_t>>& bytes, int64_t limit);
// a group cut into sub-groups runs each through the one-launch path only if there are several and each has two batches or more
// (a sub-group of ONE batch would take the per-batch path: nothing gained -- e.g. ten 1 GB batches)
bool sub_groups_of_two(const std::vector<size_t>& cuts);

// ---- the tables of the concat kernels ------------------------------------------------------------------------------------------
// One block of 64-bit words: [row_at (nb + 1)], then per column [src nb] [aux nb, byte_at nb + 1 | Utf8] [bitoff nb | Boolean]
// [vsrc nb, vbitoff nb | a column with nulls in any batch].  0 = the column has no such table (word 0 is row_at's).
struct ConcatCol { size_t src = 0, aux = 0, bitoff = 0, byte_at = 0, vsrc = 0, vbitoff = 0; bool validity = false; int utf8_k = -1; };
struct ConcatLayout { std::vector<ConcatCol> cols; size_t words = 0; };
ConcatLayout layout_concat(const std::vector<GroupCol>& schema, size_t nb, const std::vector<char>& has_nulls);

}  // namespace chq
