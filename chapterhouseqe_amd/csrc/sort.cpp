// sort.cpp -- ORDER BY on the device (chq_sort_record / chq_sort_records).
//
// Every sort key becomes one or more u64 key words whose unsigned order is the key's order (direction applied, nulls
// placed by a word of their own).  The words of all keys are radix-sorted least significant first -- the last key's
// least significant word first -- each by a stable LSD radix sort of 8-bit digits over (word, row id) pairs, so the row
// ids after the last word are the stable lexicographic order.  The first word is read in place from the column; later
// words are gathered through the permutation so far.  One read-back per word (its 8 digit histograms) decides which
// digit passes can be skipped: a digit in which every key falls in one bucket moves nothing.  DESIGN.md section 3.6.
#include <algorithm>
#include <cstring>
#include <string>

#include "sort.hpp"

namespace chq {
namespace {

constexpr int64_t kMaxSortRows = (int64_t)1 << 32;   // row ids are u32

// The key words of one sort key, least significant first (buffers and permutation are filled in by the caller).
std::vector<SortNormParams> key_words(Context& ctx, const Column& c, const SortKeyArg& k, int64_t n) {
  SortNormParams base{};
  base.n = n;
  base.invert = k.descending ? ~0ull : 0ull;
  base.nulls_first = k.nulls_first ? 1 : 0;
  const bool nulls = c.validity && c.null_count != 0;
  base.validity = nulls ? c.validity : nullptr;
  base.bit_offset = c.offset;
  base.values = (const uint8_t*)c.values0();
  base.width = c.width;
  std::vector<SortNormParams> words;
  auto add = [&](int kind, int width = 0, int64_t chunk = 0) {
    SortNormParams w = base;
    w.kind = kind;
    if (width) w.width = width;
    w.chunk = chunk;
    words.push_back(w);
  };
  const std::string& f = c.format;
  switch (c.type) {
    case T_BOOL: add(SW_BOOL); break;
    case T_I8: case T_I16: case T_I32: case T_I64: add(SW_SIGNED); break;
    case T_U8: case T_U16: case T_U32: case T_U64: add(SW_UNSIGNED); break;
    case T_F16: case T_F32: case T_F64: add(SW_FLOAT); break;
    case T_UTF8: {
      // (padded bytes, length) is the bytewise order: equal zero-padded bytes leave the shorter string, a proper prefix,
      // first.  Chunks of 8 bytes, the last chunk least significant; the length below every chunk.
      add(SW_UTF8_LEN);
      uint32_t maxlen = 0;
      if (c.data && n > 0) {
        BufferPtr d = make_device_buffer(16, ctx.device);
        check_hip(hipMemsetAsync(d->ptr, 0, 4, ctx.stream), "hipMemsetAsync");
        SortMaxLenParams mp{(const int32_t*)c.values0(), n, (uint32_t*)d->ptr};
        check_hip(launch_sort_utf8_maxlen(mp, std::max(1, ctx.num_cus) * 8, ctx.stream), "launch sort_utf8_maxlen_kernel");
        ++ctx.stats.launches;
        check_hip(hipMemcpyAsync(&maxlen, d->ptr, 4, hipMemcpyDeviceToHost, ctx.stream), "read back max length");
        check_hip(hipStreamSynchronize(ctx.stream), "hipStreamSynchronize");
      }
      base.data = c.data;
      for (int64_t ch = ((int64_t)maxlen + 7) / 8 - 1; ch >= 0; --ch) add(SW_UTF8_CHUNK, 0, ch);
      break;
    }
    case T_FIXED_OPAQUE:
      if (orders_as_signed(c)) {
        add(SW_SIGNED);
      } else if (f.rfind("d:", 0) == 0 && c.width == 16) {
        add(SW_DEC_LO, 8); add(SW_DEC_HI, 8);
      } else {
        throw ChqError{CHQ_ERR_NOT_SUPPORTED, "sort key '" + c.name + "' has Arrow type '" + f + "', which has no order in this build"};
      }
      break;
    default: throw ChqError{CHQ_ERR_NOT_SUPPORTED, "sort key '" + c.name + "' has a type without an order in this build"};
  }
  if (nulls) add(SW_NULL_FLAG);
  return words;
}

}  // namespace

// temporal types order as their signed integers, decimals of up to 8 bytes as signed integers of their width
bool orders_as_signed(const Column& c) {
  const std::string& f = c.format;
  return c.type == T_FIXED_OPAQUE &&
         (f == "tdD" || f == "tts" || f == "ttm" || f == "tdm" || f == "ttu" || f == "ttn" || f.rfind("ts", 0) == 0 ||
          f.rfind("tD", 0) == 0 || (f.rfind("d:", 0) == 0 && c.width <= 8));
}

// the key types of ORDER BY (key_words above), which JOIN and the hash partitioning share
bool sortable(const Column& c) {
  switch (c.type) {
    case T_BOOL: case T_I8: case T_I16: case T_I32: case T_I64: case T_U8: case T_U16: case T_U32: case T_U64:
    case T_F16: case T_F32: case T_F64: case T_UTF8:
      return true;
    case T_FIXED_OPAQUE: return orders_as_signed(c) || (c.format.rfind("d:", 0) == 0 && c.width == 16);
    default: return false;
  }
}

// the column an argument names: the resolver of compute_value (plan.cpp), which must come back with a bare column
int resolve_key(const Expr& e, const std::vector<PlanColumn>& pcols, int64_t nrows, const std::string& what) {
  if (e.kind != Expr::IDENT && e.kind != Expr::COMPOUND)
    throw ChqError{CHQ_ERR_NOT_SUPPORTED, what + " must be a column, not " + (e.text.empty() ? std::string("an expression") : e.text)};
  TypedExpr te = type_expr(e, pcols, std::max<int64_t>(nrows, 2), false);
  if (te.pending_code) throw ChqError{te.pending_code, te.pending_msg};
  const Node& root = te.at(te.root);
  if (root.kind != Node::COL) throw ChqError{CHQ_ERR_NOT_SUPPORTED, "a sort key must be a column"};
  return root.col;
}

// out row i = in row perm[i] (perm null: identity) for rows [0, m), on the device; pad: perm[i] may be kSortNoRow (a null row)
Column gather_column(Context& ctx, const Column& c, const uint32_t* perm, int64_t m, uint64_t* ones, Traffic& t, bool pad) {
  Column o;
  o.name = c.name; o.format = c.format; o.type = c.type; o.width = c.width; o.nullable = c.nullable || pad;
  o.length = m; o.offset = 0; o.null_count = 0;
  auto bits = [&](const uint8_t* in, int64_t bit_offset, uint64_t* count) {
    BufferPtr b = make_device_buffer((size_t)((m + 31) / 32) * 4 + 16, ctx.device);
    SortGatherParams g{};
    g.perm = perm; g.m = m; g.in = in; g.in_bit_offset = bit_offset; g.out = (uint8_t*)b->ptr; g.ones = count;
    if (m > 0) { check_hip(launch_sort_gather_bits(g, ctx.stream, pad), "launch sort_gather_bits_kernel"); ++ctx.stats.launches; }
    t.read += m * 4 + (m + 7) / 8; t.written += (m + 7) / 8;
    o.owned.push_back(b);
    return (const uint8_t*)b->ptr;
  };
  if (pad || (c.validity && c.null_count != 0)) {   // (pad: the source's bitmap, if it has one, and the padding)
    o.validity = bits(c.live_validity(), c.offset, ones);
    o.null_count = -1;   // set from `ones` once read back
  }
  if (c.type == T_BOOL) {
    o.values = bits(c.values, c.offset, nullptr);
  } else if (c.type == T_UTF8) {
    BufferPtr offs = make_device_buffer((size_t)(m + 1) * 4 + 16, ctx.device);
    o.values = (const uint8_t*)offs->ptr; o.owned.push_back(offs);
    int64_t total = 0;
    SortGatherParams g{};
    g.perm = perm; g.m = m; g.in = (const uint8_t*)c.values0(); g.out = (uint8_t*)offs->ptr; g.in_data = c.data;
    g.ntiles = (m + kSortTile - 1) / kSortTile;
    if (m == 0 || !c.data) {   // (no data buffer: every string is empty)
      check_hip(hipMemsetAsync(offs->ptr, 0, (size_t)(m + 1) * 4, ctx.stream), "hipMemsetAsync");
    } else {
      BufferPtr sums = make_device_buffer((size_t)(g.ntiles + 1) * 8 + 16, ctx.device);
      g.tile_sums = (uint64_t*)sums->ptr;
      check_hip(launch_sort_utf8_sizes(g, ctx.stream, pad), "launch sort_utf8_tile_sums_kernel");
      ctx.stats.launches += 2;
      uint64_t tot = 0;
      check_hip(hipMemcpyAsync(&tot, g.tile_sums + g.ntiles, 8, hipMemcpyDeviceToHost, ctx.stream), "read back Utf8 bytes");
      check_hip(hipStreamSynchronize(ctx.stream), "hipStreamSynchronize");
      total = (int64_t)tot;
      if (total > INT32_MAX)
        throw ChqError{CHQ_ERR_ARROW_INVALID_ARGUMENT, "Utf8 column '" + c.name + "' of the sorted output would hold " + std::to_string(total) +
                                                       " bytes, more than int32 offsets can address"};
      BufferPtr data = make_device_buffer((size_t)total + 16, ctx.device);
      g.out_data = (uint8_t*)data->ptr;
      o.data = (const uint8_t*)data->ptr; o.owned.push_back(data);
      check_hip(launch_sort_utf8_copy(g, ctx.stream, pad), "launch sort_utf8_copy_kernel");
      ctx.stats.launches += 2;
      t.read += m * 4 * 3 + total; t.written += (m + 1) * 4 + total;
    }
    if (!o.data) {
      BufferPtr data = make_device_buffer(16, ctx.device);
      o.data = (const uint8_t*)data->ptr; o.owned.push_back(data);
    }
    o.data_bytes = total;
  } else {
    BufferPtr v = make_device_buffer((size_t)(m * c.width) + 16, ctx.device);
    SortGatherParams g{};
    g.perm = perm; g.m = m; g.in = (const uint8_t*)c.values0(); g.out = (uint8_t*)v->ptr; g.width = c.width;
    if (m > 0) { check_hip(launch_sort_gather_fixed(g, ctx.stream, pad), "launch sort_gather_fixed_kernel"); ++ctx.stats.launches; }
    t.read += m * (4 + c.width); t.written += m * c.width;
    o.values = (const uint8_t*)v->ptr; o.owned.push_back(v);
  }
  return o;
}

// the permutation of rows [0, n) that orders `rec` by `keys` (null: identity -- no key, or fewer than 2 rows)
BufferPtr sort_permutation(Context& ctx, const Batch& rec, const std::vector<int>& cols, const std::vector<SortKeyArg>& keys, Traffic& t) {
  const int64_t n = rec.nrows;
  if (n < 2 || cols.empty()) return nullptr;
  const int64_t ntiles = (n + kSortTile - 1) / kSortTile;
  BufferPtr kb[2] = {make_device_buffer((size_t)n * 8 + 16, ctx.device), make_device_buffer((size_t)n * 8 + 16, ctx.device)};
  BufferPtr vb[2] = {make_device_buffer((size_t)n * 4 + 16, ctx.device), make_device_buffer((size_t)n * 4 + 16, ctx.device)};
  BufferPtr hist = make_device_buffer(8 * 256 * 4, ctx.device);
  BufferPtr tiles = make_device_buffer((size_t)ntiles * 256 * 4 + 16, ctx.device);
  std::vector<uint32_t> h(8 * 256);
  int pv = -1;   // vb[pv] holds the permutation so far (-1: identity)
  for (size_t ki = cols.size(); ki-- > 0;) {
    const Column& c = rec.cols[(size_t)cols[ki]];
    for (SortNormParams w : key_words(ctx, c, keys[ki], n)) {
      const int vo = pv == 0 ? 1 : 0;
      w.perm = pv < 0 ? nullptr : (const uint32_t*)vb[pv]->ptr;
      w.keys = (uint64_t*)kb[0]->ptr;
      w.vals = (uint32_t*)vb[vo]->ptr;
      check_hip(launch_sort_norm(w, ctx.stream), "launch sort_norm_kernel");
      t.read += n * (pv < 0 ? 0 : 4) + n * (w.kind == SW_UTF8_CHUNK ? 16 : std::max(1, w.width));
      t.written += n * 12;
      check_hip(hipMemsetAsync(hist->ptr, 0, 8 * 256 * 4, ctx.stream), "hipMemsetAsync");
      SortHistParams hp{(const uint64_t*)kb[0]->ptr, n, (uint32_t*)hist->ptr};
      check_hip(launch_sort_hist(hp, std::max(1, ctx.num_cus) * 8, ctx.stream), "launch sort_hist_kernel");
      ctx.stats.launches += 2;
      t.read += n * 8;
      check_hip(hipMemcpyAsync(h.data(), hist->ptr, 8 * 256 * 4, hipMemcpyDeviceToHost, ctx.stream), "read back histograms");
      check_hip(hipStreamSynchronize(ctx.stream), "hipStreamSynchronize");
      std::vector<int> digits;   // the digits in which the keys differ
      for (int b = 0; b < 8; ++b)
        if (std::none_of(h.begin() + b * 256, h.begin() + (b + 1) * 256, [n](uint32_t x) { return (int64_t)x == n; })) digits.push_back(b);
      int ck = 0, cv = vo;
      for (size_t di = 0; di < digits.size(); ++di) {
        const bool last = di + 1 == digits.size();
        SortPassParams pp{};
        pp.keys_in = (const uint64_t*)kb[ck]->ptr; pp.vals_in = (const uint32_t*)vb[cv]->ptr;
        pp.keys_out = last ? nullptr : (uint64_t*)kb[1 - ck]->ptr; pp.vals_out = (uint32_t*)vb[1 - cv]->ptr;
        pp.n = n; pp.ntiles = ntiles; pp.tile_counts = (uint32_t*)tiles->ptr;
        pp.digit_hist = (const uint32_t*)hist->ptr + 256 * digits[di]; pp.shift = 8 * digits[di];
        check_hip(launch_sort_pass(pp, ctx.stream), "launch sort_count/scan/scatter_kernel");
        ctx.stats.launches += 3;
        t.read += n * 8 + ntiles * 256 * 4 * 2 + n * 12;
        t.written += ntiles * 256 * 4 * 2 + n * (last ? 4 : 12);
        ck = 1 - ck; cv = 1 - cv;
      }
      pv = cv;
    }
  }
  return vb[pv];
}

Batch sort_records(Context& ctx, std::vector<Batch>& in, const chq_table_aliases* aliases, const std::vector<SortKeyArg>& keys,
                   int64_t limit) {
  if (in.empty()) throw ChqError{CHQ_ERR_ARROW_INVALID_ARGUMENT, "at least one record batch is needed"};
  if (limit < -1) throw ChqError{CHQ_ERR_ARROW_INVALID_ARGUMENT, "limit must be -1 (all rows) or at least 0"};
  int64_t rows = 0;
  for (const Batch& b : in) rows += b.nrows;
  if (rows >= kMaxSortRows) throw ChqError{CHQ_ERR_NOT_SUPPORTED, "a sort takes fewer than 2^32 rows per call (" + std::to_string(rows) + " given)"};
  // keys resolve against the schema before any data moves
  const auto pcols = plan_columns(in[0], aliases);
  std::vector<int> cols;
  for (const SortKeyArg& k : keys) {
    if (!k.column) throw ChqError{CHQ_ERR_INVALID_HANDLE, "null sort key column"};
    cols.push_back(resolve_key(*k.column, pcols, rows));
  }
  ctx.stats = chq_call_stats{};
  const Batch rec = join_group(ctx, in);
  const int64_t n = rec.nrows, m = limit < 0 ? n : std::min(limit, n);
  ctx.stats.rows_in = n; ctx.stats.rows_out = m; ctx.stats.tiles = (n + kSortTile - 1) / kSortTile;
  kernel_span_begin(ctx);
  Traffic t;
  const BufferPtr perm_buf = m > 0 ? sort_permutation(ctx, rec, cols, keys, t) : nullptr;
  const uint32_t* perm = perm_buf ? (const uint32_t*)perm_buf->ptr : nullptr;
  Batch out;
  out.nrows = m; out.on_device = true; out.device_id = ctx.device;
  BufferPtr ones = make_device_buffer(rec.cols.size() * 8 + 16, ctx.device);
  check_hip(hipMemsetAsync(ones->ptr, 0, rec.cols.size() * 8, ctx.stream), "hipMemsetAsync");
  for (size_t ci = 0; ci < rec.cols.size(); ++ci)
    out.cols.push_back(gather_column(ctx, rec.cols[ci], perm, m, (uint64_t*)ones->ptr + ci, t));
  fill_null_counts(out.cols, m, finish_call(ctx, ones->ptr, rec.cols.size(), t));
  return out;
}

std::vector<uint64_t> finish_call(Context& ctx, const void* words, size_t n, const Traffic& t, const char* what) {
  kernel_span_end(ctx);
  std::vector<uint64_t> h(n);
  if (n) check_hip(hipMemcpyAsync(h.data(), words, n * 8, hipMemcpyDeviceToHost, ctx.stream), what);
  check_hip(hipStreamSynchronize(ctx.stream), "hipStreamSynchronize");
  ctx.stats.kernel_ns += kernel_span_ns(ctx);
  ctx.stats.bytes_read_alg = t.read; ctx.stats.bytes_written_alg = t.written;
  return h;
}

void fill_null_counts(std::vector<Column>& cols, int64_t rows, const std::vector<uint64_t>& ones) {
  for (size_t ci = 0; ci < cols.size(); ++ci)
    if (cols[ci].null_count < 0) cols[ci].null_count = rows - (int64_t)ones[ci];
}

}  // namespace chq
