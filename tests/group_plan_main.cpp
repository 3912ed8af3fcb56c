// The batch-group filter's planning unit alone, under the host sanitizers (tests/test_group_plan_host.py builds and runs this).
// argv[1] is a text file of group descriptions:
//   chunk <bytes>                                     option group_chunk_bytes of every case
//   dim <name> <value> ...                            the values a `cross` line runs over: tile_kind mode fixed utf8 bool nulls refs
//   group <name> <big> <rows of batch 0> <rows of batch 1> ...
//   cross <group>                                     every combination of the dims, device-resident, default options
//   case <group> <tile_kind> <mode> <fixed> <utf8> <bool> <nulls> <refs> <wide> <residency> <group_bits> <fold_utf8> <group_fold> <flaw>
// Every case is planned as group.cpp does it -- eligibility, tiling, table layout, the table itself, the fold's size rule, the
// chunk cuts, the concat tables -- checked against the invariants the kernels rely on (16 checks a case) and printed as one
// line of text.  Pointers are never followed: they encode (role, batch, column).  A `big` group is described by its counts
// alone: no table is written for it.  Last, put_column is run on real bitmaps of host batches (15 checks).  Prints "<n> checks, <m> mismatches" last.
#include "../chapterhouseqe_amd/csrc/group_plan.cpp"

#include <cstdio>
#include <fstream>
#include <map>
#include <sstream>
#include <string>

using namespace chq;

static long n_checks = 0, n_bad = 0;
static std::string g_where;
#define CHECK(cond) do { ++n_checks; if (!(cond)) { ++n_bad; fprintf(stderr, "line %d (%s): %s\n", __LINE__, g_where.c_str(), #cond); } } while (0)

enum Role : u64 { VALUES = 1, DATA = 2, VALIDITY = 3, OFFSET = 4 };
static u64 enc(Role role, size_t b, size_t col) { return ((u64)role << 56) | ((u64)b << 16) | (u64)col; }
static const uint8_t* as_ptr(u64 v) { return (const uint8_t*)(uintptr_t)v; }
constexpr u64 kSentinel = 0xfeedfacecafebeefULL;

struct Group { bool big = false; std::vector<int64_t> rows; };
struct Case {
  std::string group;
  int tile_kind, mode, fixed, utf8, boolean, nulls, refs, wide;
  std::string residency;   // device, host, mixed
  int group_bits, fold_utf8, group_fold;
  std::string flaw;        // none, short (a batch of one row), schema (a batch of another schema), nodata (a Utf8 column without bytes)
};

static int64_t chunk_bytes = 1ll << 30;
static const int64_t kBytesPerRow[3] = {8, 24, 40};   // of the Utf8 columns, in order

// the schema of a case: fixed column 0, the Utf8 columns, the other fixed columns, the Boolean column
static std::vector<GroupCol> schema_of(const Case& c) {
  static const int64_t widths[5] = {4, 8, 2, 1, 16};
  std::vector<GroupCol> s;
  for (int i = 0; i < c.fixed; ++i) {
    s.push_back(GroupCol{T_I32, widths[i % 5]});
    if (i == 0) for (int u = 0; u < c.utf8; ++u) s.push_back(GroupCol{T_UTF8, 0});
  }
  for (int i = 0; i < c.boolean; ++i) s.push_back(GroupCol{T_BOOL, 0});
  return s;
}

static void run_case(const Case& c, const Group& grp, FILE* out) {
  const std::vector<int64_t>& rows = grp.rows;
  const size_t nb = rows.size();
  const std::vector<GroupCol> schema = schema_of(c);
  const size_t ncols = schema.size();
  const size_t n_null = std::min<size_t>((size_t)c.nulls, ncols);   // the first n_null columns carry nulls, in the odd batches
  GroupOptions opt;
  opt.tile_kind = c.tile_kind; opt.group_mode = c.mode; opt.group_bits = c.group_bits; opt.fold_utf8 = c.fold_utf8; opt.group_fold = c.group_fold;
  opt.group_chunk_bytes = chunk_bytes;

  // ---- the flat description, through put_column as the importers fill it ------------------------------------------------
  GroupLite lite;
  lite.resize(nb, ncols);
  lite.rows = rows;
  for (size_t b = 0; b < nb; ++b) {
    const bool host = c.residency == "host" || (c.residency == "mixed" && b == 1);
    uint8_t f = host ? GroupLite::GL_ON_HOST : GroupLite::GL_ON_DEVICE;
    if (c.flaw == "short" && b == nb - 1) { lite.rows[b] = 1; f |= GroupLite::GL_SHORT; }
    if (c.flaw == "schema" && b == nb - 1) f |= GroupLite::GL_SCHEMA_DIFFERS;
    for (size_t i = 0; i < ncols; ++i) {
      const bool nulls = i < n_null && b % 2 == 1;
      const bool bytes = schema[i].type == T_UTF8 && !(c.flaw == "nodata" && b == 0);
      // (device batches: null_count -1 with a bitmap counts as nulls; nothing is read)
      f |= lite.put_column(b * ncols + i, schema[i], false, nulls ? as_ptr(enc(VALIDITY, b, i)) : nullptr, nulls ? -1 : 0, lite.rows[b],
                           as_ptr(enc(VALUES, b, i)), bytes ? as_ptr(enc(DATA, b, i)) : nullptr, 0);
      lite.offset[b * ncols + i] = (int64_t)enc(OFFSET, b, i);
    }
    lite.flags[b] = f;
  }
  // put_column applied the slice offset 0: values0 is the pointer itself; the bitmap only where there are nulls
  bool put_ok = true;
  for (size_t b = 0; b < nb; ++b) for (size_t i = 0; i < ncols; ++i) {
    const size_t at = b * ncols + i;
    put_ok = put_ok && lite.values0[at] == as_ptr(enc(VALUES, b, i)) && (lite.validity[at] != nullptr) == (i < n_null && b % 2 == 1);
  }
  CHECK(put_ok);

  // ---- eligibility ----------------------------------------------------------------------------------------------------------
  const GroupPlan pl = plan_group(lite.flags, lite.rows, schema, c.residency == "host", opt);
  fprintf(out, "case %s %d %d %d %d %d %d %d %d %s %d %d %d %s | plan %d %d %d %d %d %lld %lld %zu", c.group.c_str(), c.tile_kind, c.mode, c.fixed, c.utf8,
          c.boolean, c.nulls, c.refs, c.wide, c.residency.c_str(), c.group_bits, c.fold_utf8, c.group_fold, c.flaw.c_str(), pl.per_batch, pl.plain, pl.fold,
          pl.need_bits, pl.resident, (long long)pl.total_rows, (long long)pl.max_rows, pl.fold_utf8.size());
  // (a per-batch verdict returns before the rows are summed: the tiling below is then planned from the sums taken here)
  int64_t total_rows = 0, max_rows = 0;
  for (int64_t r : lite.rows) { total_rows += r; max_rows = std::max(max_rows, r); }
  CHECK(pl.fold_utf8.size() <= (size_t)MAX_FOLD_UTF8 && pl.fold == !pl.fold_utf8.empty() && !(pl.plain && pl.fold) &&
        (pl.per_batch || (pl.total_rows == total_rows && pl.max_rows == max_rows)));

  // ---- tiling -----------------------------------------------------------------------------------------------------------------
  const GroupTiling tl = plan_tiling(c.wide != 0, opt, lite.rows, total_rows, max_rows);
  fprintf(out, " | tiling %d %lld %lld", tl.tile_kind, (long long)tl.wpb, (long long)tl.ntiles);
  const int k = tl.tile_kind;
  CHECK(k >= 0 && k <= 2 && (c.wide ? k == 2 : c.tile_kind < 0 || k == c.tile_kind));
  {
    // what the kind would be if it were left to the padding rule, and the five-fourths rule with the wave count of the kind in use
    const int kk = c.wide ? 2 : c.tile_kind >= 0 ? c.tile_kind : 0;
    const int64_t w = (max_rows + kWaveRows[kk] - 1) / kWaveRows[kk];
    const bool rule = (__int128)w * (int64_t)nb * kWaveRows[kk] * 4 <= (__int128)total_rows * 5 && (__int128)w * (int64_t)nb < (1ll << 31) - 64;
    if (tl.wpb > 0) {
      CHECK(tl.ntiles == (tl.wpb * (int64_t)nb + kWavesPerTile[k] - 1) / kWavesPerTile[k] && tl.wpb * kWaveRows[k] >= max_rows && (tl.wpb - 1) * kWaveRows[k] < max_rows);
      CHECK(c.mode == 2 || (c.mode == 0 && rule));
    } else {
      int64_t tiles = 0;
      for (int64_t r : lite.rows) tiles += (r + kTileRows[k] - 1) / kTileRows[k];
      CHECK(tl.ntiles == tiles);
      CHECK(c.mode == 1 || (c.mode == 0 && !rule));
    }
    int64_t padded = 0;
    for (int64_t r : lite.rows) padded += (r + kTileRows[0] - 1) / kTileRows[0] * kTileRows[0];
    CHECK(tl.wpb > 0 || c.wide || c.tile_kind >= 0 || k == (padded * 4 <= total_rows * 5 ? 0 : 1));
  }

  // ---- the layout of a table row -------------------------------------------------------------------------------------------
  // program refs: over the columns that are not Utf8, with repeats when there are few; outputs: every fixed-width column, the
  // first ref's last (what pick_stash does with a stashed column); bit columns as group.cpp derives them
  std::vector<int> other, refs, outs;
  for (size_t i = 0; i < ncols; ++i) if (schema[i].type != T_UTF8) other.push_back((int)i);
  for (int r = 0; r < c.refs; ++r) refs.push_back(other[(size_t)(r * 7) % other.size()]);
  for (size_t i = 0; i < ncols; ++i) if (schema[i].type != T_UTF8 && schema[i].type != T_BOOL && (refs.empty() || (int)i != refs[0])) outs.push_back((int)i);
  if (!refs.empty() && schema[(size_t)refs[0]].type != T_BOOL) outs.push_back(refs[0]);
  std::vector<BitCol> bit_cols;
  if (pl.need_bits)
    for (size_t i = 0; i < ncols; ++i) {
      if (schema[i].type == T_BOOL) bit_cols.push_back(BitCol{(int)i, false, 0});
      if (i < n_null && nb > 1) bit_cols.push_back(BitCol{(int)i, true, 0});
    }
  const size_t n_fold = pl.fold_utf8.size();
  const GroupTableLayout lay = layout_group_table(tl, nb, refs.size(), outs.size(), n_fold, pl.need_bits, bit_cols);
  fprintf(out, " | layout %d %zu %zu %zu %zu %zu %zu", lay.ok, lay.stride, lay.bits_at, lay.table_rows, lay.bytes_tbl, lay.bytes_idx, lay.bytes_cnt);
  CHECK(lay.ok == !((pl.need_bits && (tl.wpb == 0 || bit_cols.size() > 16)) || (n_fold > 0 && k == 2)));
  const size_t head = tl.wpb > 0 ? 1 : 2;
  {
    std::vector<int> used(lay.stride, 0);
    bool below = true;
    auto use = [&](size_t at, size_t n) { for (size_t q = at; q < at + n; ++q) { if (q < lay.stride) ++used[q]; else below = false; } };
    if (lay.ok) {
      use(0, head + refs.size() + outs.size() + 2 * n_fold);
      if (lay.bits_at) use(lay.bits_at, 2 * refs.size());
      if (lay.bits_at) for (const BitCol& q : bit_cols) use(q.word, 2);
    }
    bool once = below;
    for (int u : used) once = once && u == 1;
    CHECK(once);
    CHECK(!lay.ok || ((lay.bits_at == 0) == !pl.need_bits && (lay.bits_at == 0 || lay.bits_at == head + refs.size() + outs.size() + 2 * n_fold)));
    CHECK(!lay.ok || (lay.table_rows == (tl.wpb > 0 ? nb : (size_t)tl.ntiles) && lay.bytes_tbl == lay.table_rows * lay.stride * 8 &&
                      lay.bytes_idx == (tl.wpb > 0 ? 0 : nb * 8) && lay.bytes_cnt == nb * 8));
  }

  // ---- the table ------------------------------------------------------------------------------------------------------------
  bool words_ok = true, tiles_ok = true, beyond_ok = true;
  if (lay.ok && !grp.big && !pl.per_batch) {
    const size_t tbl = lay.table_rows * lay.stride, idx = lay.bytes_idx / 8, cnt = lay.bytes_cnt / 8, guard = 8;
    std::vector<u64> block(tbl + idx + cnt + guard, kSentinel);
    std::vector<const uint8_t*> in_ptr = lite.values0;   // (a staged host group would pass other pointers: here role VALUES of the same slot)
    write_group_table(lay, tl, lite, in_ptr.data(), refs, outs, pl.fold_utf8, bit_cols, block.data());
    size_t row = 0;
    for (size_t b = 0; b < nb; ++b) {
      const int64_t ntile = tl.wpb > 0 ? 1 : (lite.rows[b] + kTileRows[k] - 1) / kTileRows[k];
      for (int64_t t = 0; t < ntile; ++t, ++row) {
        if (row >= lay.table_rows) { tiles_ok = false; break; }
        const u64* w = &block[row * lay.stride];
        std::vector<u64> want(lay.stride, kSentinel);
        size_t at = 0;
        if (tl.wpb == 0) want[at++] = (u64)(t * kTileRows[k]);   // consecutive tiles from row 0, stepping by the tile's rows
        want[at++] = (u64)lite.rows[b];
        for (int r : refs) want[at++] = enc(VALUES, b, (size_t)r);
        for (int o : outs) want[at++] = enc(VALUES, b, (size_t)o);
        for (int u : pl.fold_utf8) { want[at++] = enc(VALUES, b, (size_t)u); want[at++] = enc(DATA, b, (size_t)u); }
        if (lay.bits_at) {
          for (int r : refs) want[at++] = lite.validity[b * ncols + (size_t)r] ? enc(VALIDITY, b, (size_t)r) : 0;
          for (int r : refs) want[at++] = enc(OFFSET, b, (size_t)r);
          for (const BitCol& q : bit_cols) {
            want[q.word] = q.validity ? (lite.validity[b * ncols + (size_t)q.col] ? enc(VALIDITY, b, (size_t)q.col) : 0) : enc(VALUES, b, (size_t)q.col);
            want[q.word + 1] = enc(OFFSET, b, (size_t)q.col);
          }
        }
        for (size_t q = 0; q < lay.stride; ++q) words_ok = words_ok && w[q] == want[q] && w[q] != kSentinel;
        if (tl.wpb == 0 && t == ntile - 1) {   // the tile covers the batch's last row, and the index names it
          tiles_ok = tiles_ok && t * kTileRows[k] < lite.rows[b] && (t + 1) * kTileRows[k] >= lite.rows[b] && (int64_t)block[tbl + b] == (int64_t)row;
        }
      }
    }
    tiles_ok = tiles_ok && row == lay.table_rows && (tl.wpb > 0 || (int64_t)row == tl.ntiles);
    for (size_t q = tbl + idx; q < block.size(); ++q) beyond_ok = beyond_ok && block[q] == kSentinel;   // the end offsets are the launch's to write
  }
  CHECK(words_ok);    // every word of every row set, to what the layout says lies there
  CHECK(tiles_ok);    // tile mode: a batch's tiles are consecutive, cover [0, rows) exactly; idx[b] = the tile before batch b + 1's first
  CHECK(beyond_ok);   // nothing written behind the table and the index

  // ---- sizes and cuts --------------------------------------------------------------------------------------------------------
  std::vector<std::vector<int64_t>> bytes;   // of the Utf8 columns the call would measure: the folded ones, else all of them
  const size_t n_sized = pl.fold ? n_fold : (size_t)c.utf8;
  for (size_t u = 0; u < n_sized; ++u) {
    bytes.emplace_back(nb);
    for (size_t b = 0; b < nb; ++b) bytes.back()[b] = lite.rows[b] * kBytesPerRow[u];
  }
  const FoldSizes fs = fold_sizes(bytes, total_rows, chunk_bytes);
  const std::vector<size_t> cuts = chunk_cuts(lite.rows, bytes, chunk_bytes);
  fprintf(out, " | sizes %d %d", fs.fits, fs.short_strings);
  for (int64_t cap : fs.cap) fprintf(out, " %lld", (long long)cap);
  fprintf(out, " | cuts %d", sub_groups_of_two(cuts));
  for (size_t q : cuts) fprintf(out, " %zu", q);
  {
    bool caps = fs.cap.size() == bytes.size() && (!fs.fits || fs.short_strings);
    for (size_t u = 0; u < bytes.size() && caps; ++u) caps = fs.cap[u] == total_rows * kBytesPerRow[u];
    CHECK(caps);
    bool ascend = cuts.size() >= 2 && cuts.front() == 0 && cuts.back() == nb, within = true;
    for (size_t q = 0; q + 1 < cuts.size() && ascend; ++q) {
      ascend = cuts[q] < cuts[q + 1];
      if (!ascend || cuts[q + 1] - cuts[q] == 1) continue;
      int64_t r = 0;
      for (size_t b = cuts[q]; b < cuts[q + 1]; ++b) r += lite.rows[b];
      within = within && r <= (1ll << 30);
      for (const auto& col : bytes) {
        int64_t s = 0;
        for (size_t b = cuts[q]; b < cuts[q + 1]; ++b) s += col[b];
        within = within && s <= chunk_bytes;
      }
    }
    CHECK(ascend && within);
  }

  // ---- the concat tables -------------------------------------------------------------------------------------------------------
  std::vector<char> has_nulls(ncols, 0);
  for (size_t i = 0; i < n_null && nb > 1; ++i) has_nulls[i] = 1;
  const ConcatLayout cl = layout_concat(schema, nb, has_nulls);
  fprintf(out, " | concat %zu\n", cl.words);
  {
    bool ok = cl.cols.size() == ncols;
    int n_utf8 = 0;
    std::vector<uint8_t> used(grp.big ? 0 : cl.words, 0);
    bool below = true;
    auto use = [&](size_t at, size_t n) { if (at + n > cl.words) { below = false; return; } for (size_t q = at; q < at + n && !grp.big; ++q) ++used[q]; };
    use(0, nb + 1);
    for (size_t i = 0; i < ncols && ok; ++i) {
      const ConcatCol& cc = cl.cols[i];
      const bool u = schema[i].type == T_UTF8, bo = schema[i].type == T_BOOL;
      ok = cc.validity == (has_nulls[i] != 0) && cc.utf8_k == (u ? n_utf8 : -1) && cc.src != 0 && (cc.aux != 0) == u && (cc.byte_at != 0) == u &&
           (cc.bitoff != 0) == bo && (cc.vsrc != 0) == cc.validity && (cc.vbitoff != 0) == cc.validity;
      n_utf8 += u;
      use(cc.src, nb);
      if (u) { use(cc.aux, nb); use(cc.byte_at, nb + 1); }
      if (bo) use(cc.bitoff, nb);
      if (cc.validity) { use(cc.vsrc, nb); use(cc.vbitoff, nb); }
    }
    for (uint8_t q : used) ok = ok && q == 1;
    CHECK(ok && below);
  }
}

// put_column on real memory: the host branch counts a bitmap nobody has counted, over exactly the bits of the slice (the two
// bitmaps are heap blocks of their exact size: a read past the slice's last byte is the sanitizer's to report)
static void check_put_column() {
  g_where = "put_column";
  const int64_t off = 5, len = 14;                       // bits [5, 19): bytes 0..2
  std::vector<uint8_t> all_set(3, 0xff), one_clear(3, 0xff), clear_outside(3, 0xff), values(128, 0), bytes(8, 0);
  one_clear[2] = (uint8_t)~(1u << 2);                    // bit 18, the slice's last
  clear_outside[0] = (uint8_t)~(1u << 4); clear_outside[2] = (uint8_t)~(1u << 3);   // bits 4 and 19: just outside on either side
  GroupLite g;
  g.resize(1, 8);
  const GroupCol i32{T_I32, 4}, wide{T_I64, 8}, utf8{T_UTF8, 0}, boolean{T_BOOL, 0};
  // host batches, nulls not counted (null_count -1): counted here; a bitmap with every bit of the slice set is no bitmap
  CHECK(g.put_column(0, i32, true, all_set.data(), -1, len, values.data(), nullptr, off) == 0 && g.validity[0] == nullptr);
  CHECK(g.put_column(1, i32, true, one_clear.data(), -1, len, values.data(), nullptr, off) == GroupLite::GL_NULLS && g.validity[1] == one_clear.data());
  CHECK(g.put_column(2, i32, true, clear_outside.data(), -1, len, values.data(), nullptr, off) == 0 && g.validity[2] == nullptr);
  // counted by the producer: believed, on the host and on the device alike; a device bitmap nobody counted may clear a bit
  CHECK(g.put_column(3, i32, true, all_set.data(), 0, len, values.data(), nullptr, off) == 0 && g.validity[3] == nullptr);
  CHECK(g.put_column(3, i32, true, all_set.data(), 2, len, values.data(), nullptr, off) == GroupLite::GL_NULLS && g.validity[3] == all_set.data());
  CHECK(g.put_column(4, i32, false, as_ptr(enc(VALIDITY, 0, 4)), -1, len, values.data(), nullptr, off) == GroupLite::GL_NULLS && g.validity[4] == as_ptr(enc(VALIDITY, 0, 4)));
  CHECK(g.put_column(4, i32, false, nullptr, 0, len, values.data(), nullptr, off) == 0);
  // values0 has the slice offset applied by the column's width (Utf8: its int32 offsets), a Boolean column keeps its bitmap
  CHECK(g.values0[0] == values.data() + 4 * off && g.offset[0] == off && g.data[0] == nullptr);
  CHECK(g.put_column(5, wide, true, nullptr, 0, len, values.data(), nullptr, off) == 0 && g.values0[5] == values.data() + 8 * off);
  CHECK(g.put_column(6, utf8, true, nullptr, 0, len, values.data(), bytes.data(), off) == 0 && g.values0[6] == values.data() + 4 * off && g.data[6] == bytes.data());
  CHECK(g.put_column(6, utf8, true, nullptr, 0, len, values.data(), nullptr, off) == GroupLite::GL_NO_UTF8_DATA);
  CHECK(g.put_column(7, boolean, true, one_clear.data(), -1, len, values.data(), nullptr, off) == GroupLite::GL_NULLS && g.values0[7] == values.data() && g.offset[7] == off);
  CHECK(g.put_column(7, i32, true, nullptr, -1, len, nullptr, nullptr, off) == 0 && g.values0[7] == nullptr);
  CHECK(count_nulls_host(clear_outside.data(), 4, 16) == 2 && count_nulls_host(clear_outside.data(), off, len) == 0 && count_nulls_host(one_clear.data(), 18, 1) == 1);
  const GroupLite s = g.slice(0, 1);
  CHECK(s.ncols == 8 && s.rows == g.rows && s.flags == g.flags && s.values0 == g.values0 && s.data == g.data && s.validity == g.validity && s.offset == g.offset);
}

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s <descriptions> <plans out>\n", argv[0]); return 2; }
  std::ifstream in(argv[1]);
  FILE* out = fopen(argv[2], "w");
  if (!in || !out) { fprintf(stderr, "cannot open %s or %s\n", argv[1], argv[2]); return 2; }
  std::map<std::string, Group> groups;
  std::map<std::string, std::vector<int>> dims;
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream ls(line);
    std::string word, name;
    if (!(ls >> word)) continue;
    if (word == "chunk") { ls >> chunk_bytes; continue; }
    if (word == "dim") { ls >> name; int v; while (ls >> v) dims[name].push_back(v); continue; }
    if (word == "group") { Group g; int64_t r; ls >> name >> g.big; while (ls >> r) g.rows.push_back(r); groups[name] = g; continue; }
    Case c;
    ls >> c.group;
    if (!groups.count(c.group)) { fprintf(stderr, "unknown group in: %s\n", line.c_str()); return 2; }
    if (word == "case") {
      ls >> c.tile_kind >> c.mode >> c.fixed >> c.utf8 >> c.boolean >> c.nulls >> c.refs >> c.wide >> c.residency >> c.group_bits >> c.fold_utf8 >> c.group_fold >> c.flaw;
      if (!ls) { fprintf(stderr, "bad case: %s\n", line.c_str()); return 2; }
      g_where = line;
      run_case(c, groups[c.group], out);
      continue;
    }
    if (word != "cross") { fprintf(stderr, "bad line: %s\n", line.c_str()); return 2; }
    c.wide = 0; c.residency = "device"; c.group_bits = c.fold_utf8 = c.group_fold = 1; c.flaw = "none";
    for (int tk : dims["tile_kind"]) for (int mode : dims["mode"]) for (int fixed : dims["fixed"]) for (int utf8 : dims["utf8"])
      for (int bo : dims["bool"]) for (int nulls : dims["nulls"]) for (int refs : dims["refs"]) {
        c.tile_kind = tk; c.mode = mode; c.fixed = fixed; c.utf8 = utf8; c.boolean = bo; c.nulls = nulls; c.refs = refs;
        g_where = c.group + " " + std::to_string(tk) + " " + std::to_string(mode) + " " + std::to_string(fixed) + " " + std::to_string(utf8) + " " +
                  std::to_string(bo) + " " + std::to_string(nulls) + " " + std::to_string(refs);
        run_case(c, groups[c.group], out);
      }
  }
  fclose(out);
  check_put_column();
  printf("%ld checks, %ld mismatches\n", n_checks, n_bad);
  return n_bad ? 1 : 0;
}
