// The Parquet scan's planning unit alone, under the host sanitizers (tests/test_parquet_scan_plan_host.py builds and runs this).
// argv[1] is a directory: every file named in its files.txt is opened with the library's own metadata reader, every column of
// every row group is classified and planned as parquet_scan.cpp does it, the plan is written as text into <name>.plan (a
// refusal as "error <code> <message>") and checked against the invariants the kernels rely on; then the chain construction
// and the wave cuts are checked on synthetic inputs at the edges of their rules.  Prints "<n> checks, <m> mismatches".
#include "../chapterhouseqe_amd/csrc/parquet_meta.cpp"
#include "../chapterhouseqe_amd/csrc/parquet_scan_plan.cpp"

#include <cstdio>
#include <fstream>
#include <set>

using namespace chq;

static long n_checks = 0, n_bad = 0;
static std::string g_where;
#define CHECK(cond) do { ++n_checks; if (!(cond)) { ++n_bad; fprintf(stderr, "line %d (%s): %s\n", __LINE__, g_where.c_str(), #cond); } } while (0)

// ---- one column chunk ---------------------------------------------------------------------------------------------------------
static void check_plan(const PqColumnClass& k, const PqColumnPlan& pl, const std::vector<PqPage>& pages, int64_t rows) {
  const uint64_t bound = (uint64_t)(k.compressed ? pl.image_bytes : k.csize);
  const size_t n = pl.descs.size();
  bool inside = true, running = true, tables = pl.h_nonnull.size() == n && pl.h_base.size() == n;
  int64_t row_at = 0;
  for (size_t i = 0; i < n; ++i) {
    const PqPageDesc& d = pl.descs[i];
    inside = inside && (uint64_t)d.levels_at + d.levels_len <= bound && (uint64_t)d.values_at + d.values_len <= bound;
    running = running && d.first_row == row_at;
    tables = tables && pl.h_nonnull[i] == d.num_rows && pl.h_base[i] == (uint32_t)d.first_row;
    row_at += d.num_rows;
  }
  CHECK(inside);
  CHECK(row_at == rows);
  CHECK(running);
  CHECK(tables);
  std::vector<int> seen(n, 0);
  bool listed = true;
  for (const std::vector<int32_t>* l : {&pl.plain_list, &pl.dict_list, &pl.rle_list})
    for (int32_t p : *l) { if (p < 0 || (size_t)p >= n) listed = false; else ++seen[(size_t)p]; }
  for (int s : seen) listed = listed && s == 1;
  CHECK(listed);   // the three page lists partition the descriptors
  bool src_ok = true, dst_ok = true;
  uint64_t dst_end = 0;
  for (const PqCodecJob& j : pl.jobs) {
    src_ok = src_ok && (uint64_t)j.src_at + j.src_len <= (uint64_t)k.csize;
    dst_ok = dst_ok && j.dst_at % 16 == 0 && j.dst_at >= dst_end && (uint64_t)j.dst_at + j.dst_len <= (uint64_t)pl.image_bytes;
    dst_ok = dst_ok && !j.raw && !j.image && !j.pages && !j.err && !j.index;
    dst_end = (uint64_t)j.dst_at + j.dst_len;
  }
  CHECK(src_ok && (k.compressed || pl.jobs.empty()));
  CHECK(dst_ok);   // 16-byte aligned, disjoint (ascending), inside the image; pointer fields null
  // exactly one job per V1 page of a compressed optional column carries that descriptor's index; no other job carries one
  bool patched = true;
  size_t desc = 0;
  for (const PqPage& pg : pages) {
    if (pg.type != PQ_DATA_PAGE && pg.type != PQ_DATA_PAGE_V2) continue;
    int carriers = 0;
    for (const PqCodecJob& j : pl.jobs) carriers += j.page == (int32_t)desc;
    patched = patched && carriers == (k.compressed && k.optional && pg.type == PQ_DATA_PAGE ? 1 : 0);
    ++desc;
  }
  for (const PqCodecJob& j : pl.jobs) patched = patched && j.page >= -1 && j.page < (int32_t)n;
  CHECK(patched && desc == n);
  bool walked = pl.dict_walked == (k.byte_array && !pl.dict_list.empty() && !k.compressed);
  walked = walked && pl.h_src.size() == (pl.dict_walked ? pl.dict_count : 0u) && pl.h_len.size() == pl.h_src.size();
  for (size_t i = 0; i < pl.h_src.size(); ++i)
    walked = walked && pl.h_src[i] >= pl.dict_at + 4 && (uint64_t)pl.h_src[i] + pl.h_len[i] <= (uint64_t)pl.dict_at + pl.dict_len;
  CHECK(walked);   // host-walked dictionary entries lie inside the dictionary page
}

static void plan_file(const std::string& dir, const std::string& name) {
  std::ifstream in(dir + "/" + name + ".parquet", std::ios::binary | std::ios::ate);
  std::vector<uint8_t> raw((size_t)std::max<std::streamoff>(0, in.tellg()));
  in.seekg(0);
  in.read((char*)raw.data(), (std::streamsize)raw.size());
  FILE* out = fopen((dir + "/" + name + ".plan").c_str(), "w");
  if (!out) { ++n_bad; return; }
  PqFile f;
  try { f = parquet_open(raw.data(), (int64_t)raw.size()); }
  catch (const ChqError& e) { fprintf(out, "open error %d %s\n", e.code, e.msg.c_str()); fclose(out); return; }
  for (size_t g = 0; g < f.row_groups.size(); ++g) {
    const PqRowGroup& rg = f.row_groups[g];
    fprintf(out, "rg %zu rows %lld\n", g, (long long)rg.num_rows);
    for (size_t ci = 0; ci < f.columns.size(); ++ci) {
      g_where = name + " rg " + std::to_string(g) + " column " + std::to_string(ci);
      const PqColumnSchema& cs = f.columns[ci];
      const PqColumnChunk& cc = rg.columns[ci];
      fprintf(out, "col %zu %s\n", ci, cs.name.c_str());
      try {
        const PqColumnClass k = parquet_classify_column(cs, cc, rg.num_rows, f.size);
        fprintf(out, "class format %s width %d byte_array %d boolean %d optional %d has_levels %d compressed %d first %lld csize %lld\n", k.format, k.width,
                k.byte_array, k.boolean, k.optional, k.has_levels, k.compressed, (long long)k.first, (long long)k.csize);
        // (the scan hands over exactly the chunk: a copy of its own, so that a read past it is the sanitizer's to report)
        const std::vector<uint8_t> chunk(raw.begin() + k.first, raw.begin() + k.first + k.csize);
        const PqColumnPlan pl = parquet_plan_column(k, cs, cc.pages, rg.num_rows, k.csize ? chunk.data() : nullptr);
        check_plan(k, pl, cc.pages, rg.num_rows);
        fprintf(out, "dict at %u len %u count %u walked %d image %lld\n", pl.dict_at, pl.dict_len, pl.dict_count, pl.dict_walked, (long long)pl.image_bytes);
        std::vector<const char*> list(pl.descs.size(), "?");
        for (int32_t p : pl.plain_list) list[(size_t)p] = "plain";
        for (int32_t p : pl.dict_list) list[(size_t)p] = "dict";
        for (int32_t p : pl.rle_list) list[(size_t)p] = "rle";
        for (size_t i = 0; i < pl.descs.size(); ++i) {
          const PqPageDesc& d = pl.descs[i];
          fprintf(out, "page %zu rows %u first_row %lld levels %u %u values %u %u list %s\n", i, d.num_rows, (long long)d.first_row, d.levels_at, d.levels_len,
                  d.values_at, d.values_len, list[i]);
        }
        for (const PqCodecJob& j : pl.jobs)
          fprintf(out, "job src %u %u dst %u %u codec %u page %d flags %u\n", j.src_at, j.src_len, j.dst_at, j.dst_len, j.codec, j.page, j.flags);
      } catch (const ChqError& e) {
        fprintf(out, "error %d %s\n", e.code, e.msg.c_str());
      }
    }
  }
  fclose(out);
}

// ---- chains -----------------------------------------------------------------------------------------------------------------------
static size_t count(const std::vector<PqCodecJob>& v, uint32_t dst_at, uint32_t codec) {
  size_t c = 0;
  for (const PqCodecJob& j : v) c += j.dst_at == dst_at && j.codec == codec;
  return c;
}

static void check_chains() {
  const uint32_t dst_lens[] = {3 * 65536 - 1, 3 * 65536, 3 * 65536 + 1, 20 * 65536 + 7};
  const uint32_t src_lens[] = {(512u << 10) - 1, 512u << 10, (1u << 15) + 5, (2u << 15) + 5, 2u << 15, (2u << 15) - 1, (16u << 15) + 5, (17u << 15) + 5};
  for (int64_t sb = 0; sb <= 3; ++sb) {
    g_where = "chains, snappy_blocks " + std::to_string(sb);
    std::vector<PqCodecJob> jobs;
    for (uint32_t d : dst_lens) for (uint32_t s : src_lens) for (uint32_t codec : {PQ_CODEC_SNAPPY, PQ_CODEC_STORED}) {
      PqCodecJob j{};
      j.dst_at = (uint32_t)jobs.size() * 16; j.dst_len = d; j.src_at = 7; j.src_len = s; j.codec = codec;   // (dst_at names the job)
      j.page = jobs.size() % 3 == 0 ? (int32_t)jobs.size() : -1; j.flags = j.page >= 0 ? PQ_JOB_KEEP_LEVELS : 0;
      jobs.push_back(j);
    }
    PqChain part, large;
    parquet_route_jobs(jobs.data(), jobs.size(), sb, part, large);
    size_t words[2] = {0, 0};
    std::set<uintptr_t> slices[2];
    for (const PqCodecJob& j : jobs) {
      const bool whole = sb == 0 || j.codec != PQ_CODEC_SNAPPY || j.dst_len < 3u * 65536u;
      const bool big = !whole && j.src_len >= (512u << 10);
      const PqChain& in = big ? large : part;
      const PqChain& other = big ? part : large;
      size_t elsewhere = 0;
      for (const std::vector<PqCodecJob>* v : {&other.seg, &other.index, &other.blocks, &other.finish}) for (const PqCodecJob& o : *v) elsewhere += o.dst_at == j.dst_at;
      CHECK(elsewhere == 0);
      if (whole) {   // one job, as it came
        size_t indexed = 0;
        for (const std::vector<PqCodecJob>* v : {&in.seg, &in.index, &in.finish}) for (const PqCodecJob& o : *v) indexed += o.dst_at == j.dst_at;
        CHECK(indexed == 0 && count(in.blocks, j.dst_at, j.codec) == 1);
        for (const PqCodecJob& o : in.blocks) if (o.dst_at == j.dst_at) CHECK(o.page == j.page && o.flags == j.flags && o.index == nullptr && o.src_len == j.src_len);
        continue;
      }
      const uint32_t nblk = (j.dst_len + 65535u) / 65536u;
      uint32_t n_seg = sb == 3 ? 1u : std::min<uint32_t>(16u, j.src_len >> 15);
      if (n_seg < 2) n_seg = 0;
      CHECK(count(in.blocks, j.dst_at, PQ_CODEC_SNAPPY_BLOCK) == nblk && count(in.blocks, j.dst_at, PQ_CODEC_SNAPPY) == 0);
      CHECK(count(in.finish, j.dst_at, PQ_CODEC_SNAPPY_FINISH) == 1);
      CHECK(count(in.index, j.dst_at, PQ_CODEC_SNAPPY_INDEX) == (n_seg ? 0u : 1u));
      CHECK(count(in.seg, j.dst_at, PQ_CODEC_SNAPPY_SEG) == n_seg && count(in.index, j.dst_at, PQ_CODEC_SNAPPY_RESOLVE) == n_seg);
      // every job of the page points at one slice of the table; the FINISH job keeps the page and flags, the others drop them
      uintptr_t slice = ~(uintptr_t)0;
      bool same = true, numbered = true;
      std::set<uint32_t> blocks_seen, segs_seen;
      for (const std::vector<PqCodecJob>* v : {&in.seg, &in.index, &in.blocks, &in.finish}) for (const PqCodecJob& o : *v) {
        if (o.dst_at != j.dst_at) continue;
        if (slice == ~(uintptr_t)0) slice = (uintptr_t)o.index;
        same = same && (uintptr_t)o.index == slice && o.src_len == j.src_len && o.dst_len == j.dst_len;
        if (o.codec == PQ_CODEC_SNAPPY_FINISH) same = same && o.page == j.page && o.flags == j.flags;
        else same = same && o.page == -1 && o.flags == (sb == 2 ? (uint32_t)PQ_JOB_FORCE_FALLBACK : 0u);
        if (o.codec == PQ_CODEC_SNAPPY_BLOCK) numbered = numbered && o.block < nblk && blocks_seen.insert(o.block).second;
        if (o.codec == PQ_CODEC_SNAPPY_SEG) numbered = numbered && (o.block >> 16) == n_seg && (o.block & 0xffff) < n_seg && segs_seen.insert(o.block).second;
        if (o.codec == PQ_CODEC_SNAPPY_INDEX) numbered = numbered && o.block == 0;
      }
      CHECK(same);
      CHECK(numbered && blocks_seen.size() == nblk && segs_seen.size() == n_seg);
      CHECK(slice % sizeof(uint32_t) == 0 && slices[big].insert(slice).second);
      words[big] += nblk + 2 + 4 * PQ_SNAPPY_SEGMENTS;
    }
    // slices: disjoint and of the stated size = laid end to end in the order the pages were added
    for (int b = 0; b < 2; ++b) {
      const PqChain& ch = b ? large : part;
      CHECK(ch.words == words[b]);
      size_t at = 0;
      bool tiled = true;
      for (const PqCodecJob& o : ch.finish) { tiled = tiled && (uintptr_t)o.index == at * sizeof(uint32_t); at += (o.dst_len + 65535u) / 65536u + 2 + 4 * PQ_SNAPPY_SEGMENTS; }
      CHECK(tiled && at == ch.words);
      const std::vector<PqCodecJob> flat = ch.flat();
      bool ordered = flat.size() == ch.seg.size() + ch.index.size() + ch.blocks.size() + ch.finish.size();
      size_t q = 0;
      for (const std::vector<PqCodecJob>* v : {&ch.seg, &ch.index, &ch.blocks, &ch.finish}) for (const PqCodecJob& o : *v) { ordered = ordered && q < flat.size() && memcmp(&flat[q], &o, sizeof o) == 0; ++q; }
      CHECK(ordered);
    }
    CHECK(sb == 0 ? large.finish.empty() && part.finish.empty() : !large.finish.empty() && !part.finish.empty());
  }
}

// ---- waves ------------------------------------------------------------------------------------------------------------------------
static void check_waves() {
  g_where = "waves";
  const int64_t G = (int64_t)1 << 30;
  typedef std::vector<int64_t> B;
  typedef std::vector<int> C;
  CHECK(parquet_wave_cuts(B{}) == C{0});
  CHECK(parquet_wave_cuts(B{2 * G}) == (C{0, 1}));                       // over 1 GiB: a wave alone
  CHECK(parquet_wave_cuts(B{1, 2 * G, 1}) == (C{0, 1, 2, 3}));
  CHECK(parquet_wave_cuts(B{G / 2, G / 2}) == (C{0, 2}));                // exactly 1 GiB fits
  CHECK(parquet_wave_cuts(B{G / 2, G / 2 + 1}) == (C{0, 1, 2}));         // one byte more cuts
  CHECK(parquet_wave_cuts(B{G, 0, 0, 1, G - 1, 1}) == (C{0, 3, 5, 6}));
  CHECK(parquet_wave_cuts(B(40, 0)) == (C{0, 40}));
  uint64_t seed = 88172645463325252ull;
  for (int round = 0; round < 50; ++round) {   // no gap, no overlap, every wave full: the next row group would not fit
    B bytes((size_t)(1 + round % 17));
    for (int64_t& b : bytes) { seed ^= seed << 13; seed ^= seed >> 7; seed ^= seed << 17; b = (int64_t)(seed % (uint64_t)(G / 2 * 3)); }
    const C cuts = parquet_wave_cuts(bytes);
    bool ok = cuts.front() == 0 && cuts.back() == (int)bytes.size();
    for (size_t w = 0; ok && w + 1 < cuts.size(); ++w) {
      ok = cuts[w] < cuts[w + 1];
      int64_t sum = 0;
      for (int g = cuts[w]; g < cuts[w + 1]; ++g) sum += bytes[(size_t)g];
      ok = ok && (sum <= G || cuts[w + 1] - cuts[w] == 1) && (cuts[w + 1] == (int)bytes.size() || sum + bytes[(size_t)cuts[w + 1]] > G);
    }
    CHECK(ok);
  }
  CHECK(parquet_inflate_parts(1) == 1 && parquet_inflate_parts(5) == 1 && parquet_inflate_parts(6) == 2 && parquet_inflate_parts(11) == 2 &&
        parquet_inflate_parts(12) == 3 && parquet_inflate_parts(1000) == 3);
  for (size_t n = 1; n <= 40; ++n) {   // the part boundaries cover every row group once: n_parts parts, none empty, the last ends the wave
    const size_t n_parts = parquet_inflate_parts(n);
    size_t part = 0, in_part = 0;
    bool ok = true;
    for (size_t j = 0; j < n; ++j) {
      ++in_part;
      if (!parquet_part_ends(j, n_parts, n, part)) continue;
      ok = ok && in_part > 0 && part < n_parts;
      ++part; in_part = 0;
    }
    CHECK(ok && part == n_parts && in_part == 0);
  }
  size_t first_of[3] = {0, 0, 0}, part = 0;
  for (size_t j = 0; j < 12; ++j) if (parquet_part_ends(j, 3, 12, part)) { ++part; if (part < 3) first_of[part] = j + 1; }
  CHECK(first_of[1] == 4 && first_of[2] == 8);
}

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s <directory with files.txt>\n", argv[0]); return 2; }
  std::ifstream names(std::string(argv[1]) + "/files.txt");
  std::string name;
  while (std::getline(names, name)) if (!name.empty()) plan_file(argv[1], name);
  check_chains();
  check_waves();
  printf("%ld checks, %ld mismatches\n", n_checks, n_bad);
  return n_bad ? 1 : 0;
}
