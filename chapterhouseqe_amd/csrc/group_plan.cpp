// group_plan.cpp -- the batch-group filter's host plans: every decision of a group call that needs no device (group_plan.hpp).
// Standard headers only: tests/group_plan_main.cpp runs it on the CPU, under the host sanitizers.
#include "group_plan.hpp"

#include <algorithm>

namespace chq {

// ---- GroupLite ---------------------------------------------------------------------------------------------------------------
uint8_t GroupLite::put_column(size_t at, GroupCol kind, bool on_host, const uint8_t* bitmap, int64_t null_count, int64_t length,
                              const uint8_t* values, const uint8_t* bytes, int64_t off) {
  uint8_t f = 0;
  // nulls: a device batch with a bitmap and null_count != 0 counts as having them; a host batch that has not counted
  // (null_count < 0) is counted here, and a bitmap with every bit set is no bitmap
  bool nulls = bitmap && null_count != 0;
  if (nulls && on_host && null_count < 0) nulls = count_nulls_host(bitmap, off, length) != 0;
  if (nulls) { f |= GL_NULLS; validity[at] = bitmap; }
  if (kind.type == T_UTF8 && !bytes) f |= GL_NO_UTF8_DATA;
  values0[at] = !values || kind.type == T_BOOL ? values : values + (int64_t)(kind.type == T_UTF8 ? 4 : kind.width) * off;
  data[at] = bytes;
  offset[at] = off;
  return f;
}

GroupLite GroupLite::slice(size_t b0, size_t b1) const {
  GroupLite s;
  s.ncols = ncols;
  s.rows.assign(rows.begin() + b0, rows.begin() + b1);
  s.flags.assign(flags.begin() + b0, flags.begin() + b1);
  s.values0.assign(values0.begin() + b0 * ncols, values0.begin() + b1 * ncols);
  s.data.assign(data.begin() + b0 * ncols, data.begin() + b1 * ncols);
  s.validity.assign(validity.begin() + b0 * ncols, validity.begin() + b1 * ncols);
  s.offset.assign(offset.begin() + b0 * ncols, offset.begin() + b1 * ncols);
  return s;
}

// ---- eligibility -------------------------------------------------------------------------------------------------------------
// The facts were gathered per batch at import (GroupLite::set / set_from_arrow, on the pool's threads): here one pass over
// nb flag bytes and nb row counts, for host and device groups alike.
GroupPlan plan_group(const std::vector<uint8_t>& flags, const std::vector<int64_t>& rows, const std::vector<GroupCol>& schema,
                     bool host_in, const GroupOptions& opt) {
  const bool fits = (int)schema.size() <= MAX_OUT;
  GroupPlan pl;
  pl.host_in = host_in;
  bool has_bool = false, has_utf8 = false;
  for (const GroupCol& c : schema) { has_bool |= c.type == T_BOOL; has_utf8 |= c.type == T_UTF8; }
  uint8_t any = 0, all = 0xff;
  for (uint8_t f : flags) { any |= f; all &= f; }
  if (any & (GroupLite::GL_SHORT | GroupLite::GL_SCHEMA_DIFFERS)) { pl.per_batch = true; return pl; }
  pl.all_host = (all & GroupLite::GL_ON_HOST) != 0;
  pl.all_device = (all & GroupLite::GL_ON_DEVICE) != 0;
  pl.resident = pl.host_in ? pl.all_host : pl.all_device;   // (a mixed group, or a batch on another GPU: the per-batch loop)
  // validity bitmaps and Boolean columns ride along in the one-launch path when the group is wave-packed (decided with
  // the table): their bitmaps are compacted by bit_compact_group_kernel behind the main kernel
  pl.need_bits = has_bool || (any & GroupLite::GL_NULLS);
  pl.plain = fits && !has_utf8 && (!pl.need_bits || (pl.all_device && opt.group_bits));
  // `foldable`: device-resident fixed-width or Utf8 columns -- short-string Utf8 columns can then be filtered straight out
  // of the batches by the one-launch path (their offsets and bytes per batch ride in the group table)
  const bool foldable = fits && opt.fold_utf8 && opt.group_fold && pl.all_device && !(any & GroupLite::GL_NO_UTF8_DATA) &&
                        (!pl.need_bits || opt.group_bits);
  for (int64_t r : rows) { pl.total_rows += r; pl.max_rows = std::max(pl.max_rows, r); }
  if (!pl.plain && foldable) {
    for (size_t i = 0; i < schema.size(); ++i) if (schema[i].type == T_UTF8) pl.fold_utf8.push_back((int)i);
    pl.fold = !pl.fold_utf8.empty() && (int)pl.fold_utf8.size() <= MAX_FOLD_UTF8 && pl.total_rows < (1ll << 31) - 64;
    if (!pl.fold) pl.fold_utf8.clear();
  }
  return pl;
}

// ---- tiling ------------------------------------------------------------------------------------------------------------------
// Wave-granular packing when the batches are near-uniform (every batch gets the wave count of the longest one and
// at most a fifth of the waves idle); otherwise whole tiles per batch, described by a per-tile table.
GroupTiling plan_tiling(bool wide_or_temps, const GroupOptions& opt, const std::vector<int64_t>& rows, int64_t total_rows, int64_t max_rows) {
  const int64_t nb = (int64_t)rows.size();
  GroupTiling t;
  int tile_kind = wide_or_temps ? 2 : opt.tile_kind >= 0 ? (int)opt.tile_kind : -1;
  {
    const int k = tile_kind < 0 ? 0 : tile_kind;
    const int64_t w = (max_rows + kWaveRows[k] - 1) / kWaveRows[k];
    const bool packs = w * nb * kWaveRows[k] * 4 <= total_rows * 5 && w * nb < (1ll << 31) - 64;
    if ((opt.group_mode != 1 && packs) || opt.group_mode == 2) { t.wpb = w; tile_kind = k; }
  }
  if (tile_kind < 0) {   // the large tile unless padding every batch to a multiple of it idles more than a quarter of the lanes
    int64_t padded = 0;
    for (int64_t r : rows) padded += (r + kTileRows[0] - 1) / kTileRows[0] * kTileRows[0];
    tile_kind = padded * 4 <= total_rows * 5 ? 0 : 1;
  }
  t.tile_kind = tile_kind;
  if (t.wpb > 0) t.ntiles = (t.wpb * nb + kWavesPerTile[tile_kind] - 1) / kWavesPerTile[tile_kind];
  else for (int64_t r : rows) t.ntiles += (r + kTileRows[tile_kind] - 1) / kTileRows[tile_kind];
  return t;
}

// ---- the group table ---------------------------------------------------------------------------------------------------------
GroupTableLayout layout_group_table(const GroupTiling& tl, size_t nb, size_t n_refs, size_t n_out, size_t n_fold, bool need_bits,
                                    std::vector<BitCol>& bit_cols) {
  GroupTableLayout lay;
  const bool wave = tl.wpb > 0;
  if (need_bits && (!wave || bit_cols.size() > 16)) return lay;
  if (n_fold > 0 && tl.tile_kind == 2) return lay;
  lay.stride = (wave ? 1 : 2) + n_refs + n_out + 2 * n_fold;
  if (need_bits) {
    lay.bits_at = lay.stride;
    lay.stride += 2 * n_refs;
    for (BitCol& q : bit_cols) { q.word = lay.stride; lay.stride += 2; }
  }
  lay.table_rows = wave ? nb : (size_t)tl.ntiles;
  lay.bytes_tbl = lay.table_rows * lay.stride * 8;
  lay.bytes_idx = wave ? 0 : nb * 8;
  lay.bytes_cnt = nb * 8;
  lay.ok = true;
  return lay;
}

void write_group_table(const GroupTableLayout& lay, const GroupTiling& tl, const GroupLite& lite, const uint8_t* const* in_ptr,
                       const std::vector<int>& refs, const std::vector<int>& outs, const std::vector<int>& fold,
                       const std::vector<BitCol>& bit_cols, u64* block) {
  const size_t nb = lite.rows.size(), ncols = lite.ncols;
  const int64_t tile_rows = kTileRows[tl.tile_kind];
  u64* w = block;
  int64_t* h_idx = (int64_t*)(block + lay.table_rows * lay.stride);
  int64_t tile = 0;
  for (size_t b = 0; b < nb; ++b) {
    const int64_t rows = lite.rows[b];
    const size_t at = b * ncols;
    auto value_ptrs = [&] {   // program refs, output columns, per folded Utf8 column its offsets and bytes
      for (int c : refs) *w++ = (u64)(uintptr_t)in_ptr[at + (size_t)c];
      for (int c : outs) *w++ = (u64)(uintptr_t)in_ptr[at + (size_t)c];
      for (int c : fold) { *w++ = (u64)(uintptr_t)in_ptr[at + (size_t)c]; *w++ = (u64)(uintptr_t)lite.data[at + (size_t)c]; }
    };
    if (tl.wpb > 0) {
      *w++ = (u64)rows;
      value_ptrs();
      if (lay.bits_at) {
        for (int c : refs) *w++ = (u64)(uintptr_t)lite.validity[at + (size_t)c];
        for (int c : refs) *w++ = (u64)lite.offset[at + (size_t)c];
        for (const BitCol& q : bit_cols) {
          *w++ = (u64)(uintptr_t)(q.validity ? lite.validity[at + (size_t)q.col] : lite.values0[at + (size_t)q.col]);   // (a Boolean column's values0 is its bitmap)
          *w++ = (u64)lite.offset[at + (size_t)q.col];
        }
      }
      continue;
    }
    for (int64_t r0 = 0; r0 < rows; r0 += tile_rows, ++tile) {
      *w++ = (u64)r0; *w++ = (u64)rows;
      value_ptrs();
    }
    h_idx[b] = tile - 1;   // rows >= 2: every batch owns at least one tile
  }
}

// ---- sizes and cuts ----------------------------------------------------------------------------------------------------------
FoldSizes fold_sizes(const std::vector<std::vector<int64_t>>& bytes, int64_t total_rows, int64_t chunk_bytes) {
  FoldSizes z;
  for (const std::vector<int64_t>& per_batch : bytes) {
    int64_t cap = 0;
    for (int64_t v : per_batch) cap += v;
    z.cap.push_back(cap);
    z.short_strings = z.short_strings && cap <= total_rows * 24;
    z.fits = z.fits && cap <= total_rows * 24 && cap < 2 * chunk_bytes - 64;
  }
  return z;
}

std::vector<size_t> chunk_cuts(const std::vector<int64_t>& rows, const std::vector<std::vector<int64_t>>& bytes, int64_t limit) {
  std::vector<size_t> cuts{0};
  std::vector<int64_t> sum(bytes.size(), 0);
  int64_t at = 0;
  for (size_t b = 0; b < rows.size(); ++b) {
    bool over = at + rows[b] > (1ll << 30);
    for (size_t k = 0; k < bytes.size(); ++k) over |= sum[k] + bytes[k][b] > limit;
    if (over && b > cuts.back()) { cuts.push_back(b); std::fill(sum.begin(), sum.end(), 0); at = 0; }
    for (size_t k = 0; k < bytes.size(); ++k) sum[k] += bytes[k][b];
    at += rows[b];
  }
  cuts.push_back(rows.size());
  return cuts;
}

bool sub_groups_of_two(const std::vector<size_t>& cuts) {
  bool ok = cuts.size() > 2;
  for (size_t k = 0; k + 1 < cuts.size(); ++k) ok = ok && cuts[k + 1] - cuts[k] >= 2;
  return ok;
}

// ---- the tables of the concat kernels ----------------------------------------------------------------------------------------
ConcatLayout layout_concat(const std::vector<GroupCol>& schema, size_t nb, const std::vector<char>& has_nulls) {
  ConcatLayout lay;
  lay.cols.resize(schema.size());
  size_t words = nb + 1;
  int n_utf8 = 0;
  for (size_t c = 0; c < schema.size(); ++c) {
    ConcatCol& pl = lay.cols[c];
    pl.validity = has_nulls[c] != 0;
    pl.src = words; words += nb;
    if (schema[c].type == T_UTF8) {
      pl.aux = words; words += nb;
      pl.byte_at = words; words += nb + 1;
      pl.utf8_k = n_utf8++;
    }
    if (schema[c].type == T_BOOL) { pl.bitoff = words; words += nb; }
    if (pl.validity) { pl.vsrc = words; words += nb; pl.vbitoff = words; words += nb; }
  }
  lay.words = words;
  return lay;
}

}  // namespace chq
