// The Parquet writer's layout unit alone, under the host sanitizers (tests/test_parquet_layout_host.py builds and runs this,
// then reads every file it wrote).  What the kernels of parquet_write.hip would hand over is made here with plain loops --
// compacted non-null values, [length][bytes] strings, bit-packed Booleans, validity from bit 0, the byte prefix of every
// 4096-row block, the order-preserving statistics keys -- the layout and footer functions are called, the pieces placed with
// memcpy, and each file written into the directory argv[1].  Values are functions of the row number (the Python side has the
// same rules); internal checks: head and slice sizes sum to the chunk lengths, the pieces tile [4, footer).
#include "../chapterhouseqe_amd/csrc/parquet_layout.cpp"

#include <cmath>
#include <cstdio>
#include <functional>
#include <limits>

using namespace chq;

static long n_checks = 0, n_bad = 0;
#define CHECK(cond) do { ++n_checks; if (!(cond)) { ++n_bad; fprintf(stderr, "line %d: %s\n", __LINE__, #cond); } } while (0)

struct Col { PwChunk ch; std::vector<uint8_t> stream, levels; };
typedef std::vector<uint8_t> Bytes;
template <class T> static void put(Bytes& o, T v) { const uint8_t* p = (const uint8_t*)&v; o.insert(o.end(), p, p + sizeof v); }

static int64_t key32(int32_t b) { return b ^ (int32_t)(((uint32_t)(b >> 31)) >> 1); }
static int64_t key64(int64_t b) { return b ^ (int64_t)(((uint64_t)(b >> 63)) >> 1); }

// `value(r, stream)` appends row r's PLAIN value (Boolean: one byte); `valid`: the bitmap, or null for a column without one
static Col make_col(const std::string& name, int physical, bool optional, int64_t rows, int64_t page_rows,
                    const std::function<bool(int64_t)>* valid, const std::function<void(int64_t, Bytes&)>& value) {
  Col c;
  c.ch.name = name; c.ch.physical = physical; c.ch.optional = optional; c.ch.rows = rows;
  c.ch.has_levels = valid && rows > 0;
  if (c.ch.has_levels) c.levels.assign((size_t)(rows + 7) / 8, 0);
  const bool scanned = rows > 0 && (valid || physical == PQ_BYTE_ARRAY || physical == PQ_BOOLEAN);
  const bool want_prefix = scanned && rows > page_rows && physical != PQ_BOOLEAN;
  int64_t mn = INT64_MAX, mx = INT64_MIN, values = 0, counted = 0;
  std::string smin, smax;
  for (int64_t r = 0; r < rows; ++r) {
    if (want_prefix && r % PW_LAYOUT_BLOCK_ROWS == 0) c.ch.prefix.push_back(c.stream.size());
    if (valid && !(*valid)(r)) continue;
    if (valid) c.levels[(size_t)(r / 8)] |= (uint8_t)(1u << (r % 8));
    const size_t at = c.stream.size();
    value(r, c.stream);
    ++values;
    const uint8_t* v = c.stream.data() + at;
    int64_t k = 0;
    if (physical == PQ_BYTE_ARRAY) {
      const std::string s((const char*)v + 4, c.stream.size() - at - 4);
      if (!counted || s < smin) smin = s;   // (std::string compares as unsigned bytes)
      if (!counted || smax < s) smax = s;
      ++counted;
      continue;
    }
    if (physical == PQ_INT32) { int32_t x; memcpy(&x, v, 4); k = x; }
    else if (physical == PQ_INT64) { memcpy(&k, v, 8); }
    else if (physical == PQ_FLOAT) { float f; int32_t b; memcpy(&f, v, 4); memcpy(&b, v, 4); if (f != f) continue; k = key32(b); }
    else if (physical == PQ_DOUBLE) { double f; int64_t b; memcpy(&f, v, 8); memcpy(&b, v, 8); if (f != f) continue; k = key64(b); }
    else k = *v;
    mn = std::min(mn, k); mx = std::max(mx, k); ++counted;
  }
  if (physical == PQ_BOOLEAN) {   // the compacted bytes -> bit-packed
    Bytes bits((size_t)(values + 7) / 8, 0);
    for (int64_t i = 0; i < values; ++i) if (c.stream[(size_t)i]) bits[(size_t)(i / 8)] |= (uint8_t)(1u << (i % 8));
    c.stream = bits;
  }
  c.ch.stream_bytes = (int64_t)c.stream.size();
  c.ch.null_count = valid && rows > 0 ? rows - values : 0;
  if (counted && physical != PQ_BYTE_ARRAY) parquet_statistics_bytes(mn, mx, c.ch);
  else if (counted && smin.size() <= 4096 && smax.size() <= 4096) { c.ch.min_value = smin; c.ch.max_value = smax; c.ch.has_minmax = true; }
  return c;
}

// ---- the rules the Python side shares ---------------------------------------------------------------------------------------
static const std::function<bool(int64_t)> rule_valid = [](int64_t r) { return r % 3 != 1 && !(r >= 4096 && r < 8192); };
static const std::function<bool(int64_t)> rule_never = [](int64_t) { return false; };
static void rule_i32(int64_t r, Bytes& o) { put<uint32_t>(o, (uint32_t)r * 2654435761u); }
static void rule_i64(int64_t r, Bytes& o) { put<uint64_t>(o, (uint64_t)r * 0x9E3779B97F4A7C15ull); }
static void rule_f64(int64_t r, Bytes& o) { put<double>(o, (double)r * 0.5 - 1000.0); }
static void rule_flag(int64_t r, Bytes& o) { o.push_back((r * 7) % 11 < 5); }
static void rule_s(int64_t r, Bytes& o) {
  const uint32_t len = r % 7 == 3 ? 0 : (uint32_t)((r * 5) % 23);
  put<uint32_t>(o, len);
  for (uint32_t i = 0; i < len; ++i) o.push_back((uint8_t)('a' + (r + i) % 26));
}
// the six columns of the page-cut cases; `kind` 0 .. 5
static Col rule_col(int kind, const std::string& name, int64_t rows, int64_t page_rows) {
  switch (kind) {
    case 0: return make_col(name, PQ_INT32, false, rows, page_rows, nullptr, rule_i32);
    case 1: return make_col(name, PQ_INT64, true, rows, page_rows, nullptr, rule_i64);   // optional without a bitmap: the RLE run
    case 2: return make_col(name, PQ_DOUBLE, true, rows, page_rows, &rule_valid, rule_f64);
    case 3: return make_col(name, PQ_BYTE_ARRAY, true, rows, page_rows, &rule_valid, rule_s);
    case 4: return make_col(name, PQ_BOOLEAN, false, rows, page_rows, nullptr, rule_flag);
    default: return make_col(name, PQ_BOOLEAN, true, rows, page_rows, &rule_valid, rule_flag);
  }
}
static const char* const SIX[6] = {"req_i32", "opt_i64", "opt_f64", "s", "req_flag", "opt_flag"};
static std::vector<Col> six(int64_t rows, int64_t page_rows) {
  std::vector<Col> cols;
  for (int k = 0; k < 6; ++k) cols.push_back(rule_col(k, SIX[k], rows, page_rows));
  return cols;
}

// ---- one file: layout, footer, the pieces placed ------------------------------------------------------------------------------
static std::string g_dir;
static void write_file(const std::string& name, const std::vector<std::vector<Col>>& cols, int64_t opt_page_rows) {
  std::vector<PwGroup> groups(cols.size());
  int64_t at = 4;
  for (size_t gi = 0; gi < cols.size(); ++gi) {
    PwGroup& g = groups[gi];
    g.rows = cols[gi].empty() ? 0 : cols[gi][0].ch.rows;
    for (const Col& c : cols[gi]) g.chunks.push_back(c.ch);
    const int64_t before = at;
    parquet_layout_group(g, parquet_write_page_rows(opt_page_rows, g.rows), at);
    int64_t sum = 0;
    for (const PwChunkLayout& l : g.layout) sum += l.bytes;
    CHECK(at - before == sum && g.layout.size() == g.chunks.size());
  }
  const Bytes footer = parquet_write_footer(groups);
  Bytes img((size_t)at + footer.size() + 8, 0xEE);
  memcpy(img.data(), "PAR1", 4);
  int64_t p = 4;   // the pieces in file order: each must start where the one before ended
  for (size_t gi = 0; gi < groups.size(); ++gi) for (size_t ci = 0; ci < groups[gi].chunks.size(); ++ci) {
    const Col& c = cols[gi][ci];
    const PwChunkLayout& l = groups[gi].layout[ci];
    CHECK(l.at == p);
    int64_t rows = 0, stream = 0, total = 0;
    for (const PwPage& pg : l.pages) {
      memcpy(img.data() + p, pg.head.data(), pg.head.size()); p += (int64_t)pg.head.size();
      CHECK(pg.levels_bytes >= 0 && pg.levels_at >= 0 && pg.levels_at + pg.levels_bytes <= (int64_t)c.levels.size());
      CHECK(pg.stream_bytes >= 0 && pg.stream_at == (pg.stream_bytes ? stream : pg.stream_at) && pg.stream_at + pg.stream_bytes <= (int64_t)c.stream.size());
      if (pg.levels_bytes) { memcpy(img.data() + p, c.levels.data() + pg.levels_at, (size_t)pg.levels_bytes); p += pg.levels_bytes; }
      if (pg.stream_bytes) { memcpy(img.data() + p, c.stream.data() + pg.stream_at, (size_t)pg.stream_bytes); p += pg.stream_bytes; }
      rows += pg.rows; stream += pg.stream_bytes; total += pg.total();
    }
    CHECK(rows == c.ch.rows && stream == c.ch.stream_bytes && total == l.bytes && p == l.at + l.bytes);
  }
  CHECK(p == at);   // the pieces tile [4, footer)
  memcpy(img.data() + at, footer.data(), footer.size());
  const uint32_t flen = (uint32_t)footer.size();
  memcpy(img.data() + at + footer.size(), &flen, 4);
  memcpy(img.data() + at + footer.size() + 4, "PAR1", 4);
  FILE* f = fopen((g_dir + "/" + name + ".parquet").c_str(), "wb");
  CHECK(f && fwrite(img.data(), 1, img.size(), f) == img.size());
  if (f) fclose(f);
}

// ---- statistics: literal columns of four rows ------------------------------------------------------------------------------------
template <class T> static Col literal(const std::string& name, int physical, std::vector<T> v, std::vector<int> valid = {}) {
  const std::function<bool(int64_t)> is_valid = [&](int64_t r) { return valid[(size_t)r] != 0; };
  return make_col(name, physical, true, (int64_t)v.size(), 4096, valid.empty() ? nullptr : &is_valid,
                  [&](int64_t r, Bytes& o) { if (physical == PQ_BOOLEAN) o.push_back(v[(size_t)r] != 0); else put<T>(o, v[(size_t)r]); });
}
static std::vector<Col> statistics_columns() {
  const float inf32 = std::numeric_limits<float>::infinity(), tiny32 = std::numeric_limits<float>::denorm_min();
  const double inf64 = std::numeric_limits<double>::infinity(), tiny64 = std::numeric_limits<double>::denorm_min();
  std::vector<Col> c;
  c.push_back(literal<int32_t>("i32_extremes", PQ_INT32, {INT32_MIN, INT32_MAX, 0, -1}));
  c.push_back(literal<int64_t>("i64_extremes", PQ_INT64, {INT64_MAX, INT64_MIN, 0, -1}));
  c.push_back(literal<int32_t>("i32_only_min", PQ_INT32, {INT32_MIN, INT32_MIN, INT32_MIN, INT32_MIN}));
  c.push_back(literal<int64_t>("i64_only_max", PQ_INT64, {INT64_MAX, INT64_MAX, INT64_MAX, INT64_MAX}));
  c.push_back(literal<float>("f32_pos_zero_min", PQ_FLOAT, {0.0f, 1.0f, 2.0f, 1.0f}));
  c.push_back(literal<float>("f32_neg_zero_min", PQ_FLOAT, {-0.0f, 1.0f, 2.0f, 1.0f}));
  c.push_back(literal<float>("f32_pos_zero_max", PQ_FLOAT, {0.0f, -1.0f, -2.0f, -1.0f}));
  c.push_back(literal<float>("f32_neg_zero_max", PQ_FLOAT, {-0.0f, -1.0f, -2.0f, -1.0f}));
  c.push_back(literal<float>("f32_both_zeros", PQ_FLOAT, {-0.0f, 0.0f, -0.0f, 0.0f}));
  c.push_back(literal<float>("f32_infinities", PQ_FLOAT, {1.5f, inf32, -inf32, -2.5f}));
  c.push_back(literal<float>("f32_subnormals", PQ_FLOAT, {tiny32, -tiny32, 0.0f, -0.0f}));
  c.push_back(literal<float>("f32_nan_and_null", PQ_FLOAT, {std::nanf(""), 3.0f, -std::nanf(""), -9.0f}, {1, 1, 1, 0}));
  c.push_back(literal<double>("f64_pos_zero_min", PQ_DOUBLE, {0.0, 1.0, 2.0, 1.0}));
  c.push_back(literal<double>("f64_neg_zero_min", PQ_DOUBLE, {-0.0, 1.0, 2.0, 1.0}));
  c.push_back(literal<double>("f64_pos_zero_max", PQ_DOUBLE, {0.0, -1.0, -2.0, -1.0}));
  c.push_back(literal<double>("f64_neg_zero_max", PQ_DOUBLE, {-0.0, -1.0, -2.0, -1.0}));
  c.push_back(literal<double>("f64_both_zeros", PQ_DOUBLE, {-0.0, 0.0, -0.0, 0.0}));
  c.push_back(literal<double>("f64_infinities", PQ_DOUBLE, {1.5, inf64, -inf64, -2.5}));
  c.push_back(literal<double>("f64_subnormals", PQ_DOUBLE, {tiny64, -tiny64, 0.0, -0.0}));
  c.push_back(literal<double>("f64_only_nans", PQ_DOUBLE, {std::nan(""), -std::nan(""), std::nan(""), std::nan("")}));
  c.push_back(literal<int>("flag_mixed", PQ_BOOLEAN, {0, 1, 1, 0}));
  c.push_back(literal<int>("flag_all_false", PQ_BOOLEAN, {0, 0, 0, 0}));
  c.push_back(literal<int>("flag_all_true", PQ_BOOLEAN, {1, 1, 1, 1}));
  c.push_back(literal<int>("flag_true_under_null", PQ_BOOLEAN, {1, 0, 0, 1}, {0, 1, 1, 0}));
  c.push_back(literal<int32_t>("i32_all_null", PQ_INT32, {1, 2, 3, 4}, {0, 0, 0, 0}));
  c.push_back(literal<double>("f64_all_null", PQ_DOUBLE, {1, 2, 3, 4}, {0, 0, 0, 0}));
  c.push_back(literal<int>("flag_all_null", PQ_BOOLEAN, {1, 0, 1, 0}, {0, 0, 0, 0}));
  c.push_back(make_col("s_all_null", PQ_BYTE_ARRAY, true, 4, 4096, &rule_never, rule_s));
  return c;
}

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: parquet_layout_main DIRECTORY\n"); return 2; }
  g_dir = argv[1];
  // the page-size rule
  CHECK(parquet_write_page_rows(4096, 0) == 4096 && parquet_write_page_rows(1, 100000) == 4096 && parquet_write_page_rows(5000, 100000) == 4096);
  CHECK(parquet_write_page_rows(8191, 5) == 4096 && parquet_write_page_rows(8192, 5) == 8192 && parquet_write_page_rows(65536, 1 << 20) == 65536);
  CHECK(parquet_write_page_rows(4096, 64 * 4096) == 4096 && parquet_write_page_rows(4096, 64 * 4096 + 1) == 8192);
  CHECK(parquet_write_page_rows(65536, 64 * 65536 + 1) == 65536 + 4096 && parquet_write_page_rows(4096, (1ll << 31) - 1) == (1 << 25));
  // page cuts
  for (int64_t rows : {0, 1, 4095, 4096, 4097, 3 * 4096 + 5}) write_file("cuts_" + std::to_string(rows), {six(rows, 4096)}, 4096);
  // the 64-page widening; page sizes that round to 4096
  write_file("widened", {{rule_col(0, SIX[0], 64 * 4096 + 1, 8192)}}, 4096);
  write_file("page_rows_1", {six(4097, 4096)}, 1);
  write_file("page_rows_5000", {six(4097, 4096)}, 5000);
  // several row groups
  write_file("row_groups", {six(4097, 4096), six(0, 4096), six(1, 4096), six(8192, 4096)}, 4096);
  // Thrift forms: list headers of 15, 16 and 17 elements, a name and a bound whose lengths take a two-byte varint
  for (int n : {15, 16}) {   // (15 elements are the first list that needs the long header)
    std::vector<Col> cols;
    for (int k = 0; k < n; ++k) cols.push_back(rule_col(k % 6, "c" + std::to_string(10 + k), 5, 4096));
    write_file("schema_" + std::to_string(n), {cols}, 4096);
  }
  write_file("long_name", {{rule_col(0, std::string(130, 'n'), 5, 4096), rule_col(3, std::string(129, 'm') + "\xc3\xa9", 5, 4096)}}, 4096);
  write_file("long_bound", {{make_col("s", PQ_BYTE_ARRAY, true, 3, 4096, nullptr, [](int64_t r, Bytes& o) {
    const uint32_t len = r == 0 ? 4096 : 1;   // row 0: 4096 bytes from 'a' (the minimum), rows 1 and 2: "b", "c"
    put<uint32_t>(o, len);
    for (uint32_t i = 0; i < len; ++i) o.push_back((uint8_t)('a' + (r + i) % 26));
  })}}, 4096);
  // statistics bytes
  write_file("statistics", {statistics_columns()}, 4096);
  printf("%ld checks, %ld mismatches\n", n_checks, n_bad);
  return n_bad ? 1 : 0;
}
