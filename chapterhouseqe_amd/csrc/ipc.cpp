// ipc.cpp -- Arrow IPC *stream* encoding of one record batch with the message body in HBM.
//
// The reference serialises a batch that leaves the process with arrow-rs' ipc::writer::StreamWriter (schema message, one
// RecordBatch message, end-of-stream; src/handlers/message_handler/messages/exchange.rs:145-197) and reads it back with
// ipc::reader::StreamReader (exchange.rs:247-276).  Here the same wire format is produced for a batch that lives on the
// GPU: the two metadata flatbuffers (Schema, RecordBatch: a few hundred bytes) are built on the host, the message BODY --
// every Arrow buffer, rebased to offset 0, 64-byte aligned, back to back -- is assembled in ONE HBM allocation by device
// copies / small kernels, so a peer can receive it with a single RCCL send (or one D2H copy when it has to cross TCP).
// Decoding is the inverse: the body is moved to its destination with one copy and the columns are views into it.
//
// Format (arrow/format/{Message,Schema}.fbs, metadata version V5, little endian); flatbuffers are written and read by the
// few dozen lines below -- no dependency.  Dictionaries, compression and nested types are outside the path's scope
// (CHQ_ERR_NOT_SUPPORTED); the column kinds are those of engine.hpp: Boolean, Int8..UInt64, Float16/32/64, Utf8 and the
// fixed-width "opaque" types (date / time / timestamp / duration / decimal / fixed-size binary).
#include <cstring>

#include "engine.hpp"

namespace chq {

hipError_t launch_rebase_offsets(const int32_t* in, int32_t* out, int64_t n_plus_1, hipStream_t stream);
hipError_t launch_bit_shift_copy(const uint8_t* in, int64_t bit_offset, int64_t nbits, uint32_t* out, hipStream_t stream);
hipError_t launch_count_bits(const uint8_t* in, int64_t bit_offset, int64_t nbits, unsigned long long* out, hipStream_t stream);
hipError_t launch_validate_offsets(const int32_t* offs, int64_t n, int64_t data_len, uint32_t* flag, hipStream_t stream);

namespace {

// ---------------------------------------------------------------------------------------------------- flatbuffers: write
// Built back to front like the reference implementation: children first (higher addresses), `pos` = distance from the END.
class FlatWriter {
 public:
  FlatWriter() : buf_(1024), head_(1024) {}
  size_t size() const { return buf_.size() - head_; }
  void pad(size_t n) { reserve(n); head_ -= n; memset(&buf_[head_], 0, n); }
  void align(size_t a) { if (a > minalign_) minalign_ = a; pad((~size() + 1) & (a - 1)); }
  void prealign(size_t len, size_t a) { if (a > minalign_) minalign_ = a; pad((~(size() + len) + 1) & (a - 1)); }
  template <typename T> void push(T v) { align(sizeof(T)); reserve(sizeof(T)); head_ -= sizeof(T); memcpy(&buf_[head_], &v, sizeof(T)); }
  uint32_t string(const std::string& s) {
    prealign(s.size() + 1, 4);
    pad(1);
    reserve(s.size()); head_ -= s.size(); memcpy(&buf_[head_], s.data(), s.size());
    push<uint32_t>((uint32_t)s.size());
    return (uint32_t)size();
  }
  uint32_t offset_vector(const std::vector<uint32_t>& targets) {
    prealign(targets.size() * 4, 4);
    for (size_t i = targets.size(); i-- > 0;) { align(4); push<uint32_t>((uint32_t)(size() - targets[i] + 4)); }
    push<uint32_t>((uint32_t)targets.size());
    return (uint32_t)size();
  }
  uint32_t pair_vector(const std::vector<std::pair<int64_t, int64_t>>& v) {   // [FieldNode] / [Buffer]: structs of two longs
    prealign(v.size() * 16, 4);
    prealign(v.size() * 16, 8);
    for (size_t i = v.size(); i-- > 0;) { push<int64_t>(v[i].second); push<int64_t>(v[i].first); }
    push<uint32_t>((uint32_t)v.size());
    return (uint32_t)size();
  }
  void start_table() { fields_.clear(); }
  template <typename T> void scalar(int id, T v) { push<T>(v); fields_.push_back({(uint32_t)size(), id}); }
  void ref(int id, uint32_t target) {
    if (!target) return;
    align(4);
    push<uint32_t>((uint32_t)(size() - target + 4));
    fields_.push_back({(uint32_t)size(), id});
  }
  uint32_t end_table(uint32_t object_start) {
    align(4);
    push<int32_t>(0);   // soffset to the vtable, patched below
    const uint32_t table = (uint32_t)size();
    int maxid = -1;
    for (auto& f : fields_) maxid = std::max(maxid, f.id);
    for (int id = maxid; id >= 0; --id) {
      uint16_t off = 0;
      for (auto& f : fields_) if (f.id == id) off = (uint16_t)(table - f.pos);
      push<uint16_t>(off);
    }
    push<uint16_t>((uint16_t)(table - object_start));
    push<uint16_t>((uint16_t)((maxid + 1 + 2) * 2));
    const int32_t so = (int32_t)(size() - table);
    memcpy(&buf_[buf_.size() - table], &so, 4);
    return table;
  }
  uint32_t mark() const { return (uint32_t)size(); }
  std::vector<uint8_t> finish(uint32_t root) {
    prealign(4, std::max<size_t>(minalign_, 8));
    push<uint32_t>((uint32_t)(size() - root + 4));
    return std::vector<uint8_t>(buf_.begin() + (long)head_, buf_.end());
  }

 private:
  void reserve(size_t n) {
    if (head_ >= n) return;
    const size_t used = size(), grow = std::max(buf_.size(), n + 64);
    std::vector<uint8_t> nb(buf_.size() + grow);
    memcpy(&nb[nb.size() - used], &buf_[head_], used);
    head_ = nb.size() - used;
    buf_.swap(nb);
  }
  struct Loc { uint32_t pos; int id; };
  std::vector<uint8_t> buf_;
  size_t head_;
  size_t minalign_ = 1;
  std::vector<Loc> fields_;
};

// ----------------------------------------------------------------------------------------------------- flatbuffers: read
// Positions are byte offsets into the metadata (0 = "absent": offset 0 holds the root offset, never a table).  Every read is
// bounds-checked by subtraction, so a forged offset can neither leave the buffer nor wrap.
struct FlatReader {
  const uint8_t* base; size_t len;
  [[noreturn]] void bad() const { throw ChqError{CHQ_ERR_ARROW_INVALID_ARGUMENT, "malformed Arrow IPC metadata"}; }
  template <typename T> T rd(size_t p) const { if (p > len || len - p < sizeof(T)) bad(); T v; memcpy(&v, base + p, sizeof(T)); return v; }
  size_t follow(size_t p) const { const uint32_t o = rd<uint32_t>(p); if (o == 0 || o > len - p) bad(); return p + o; }
  size_t root() const { return follow(0); }
  size_t field(size_t t, int id) const {
    const int64_t vt = (int64_t)t - rd<int32_t>(t);
    if (vt < 0 || (uint64_t)vt > len) bad();
    const uint16_t vts = rd<uint16_t>((size_t)vt), tsize = rd<uint16_t>((size_t)vt + 2);
    if (vts < 4 || (vts & 1) || vts > len - (size_t)vt || tsize < 4 || tsize > len - t) bad();
    if (4 + 2 * id + 2 > vts) return 0;
    const uint16_t off = rd<uint16_t>((size_t)vt + 4 + 2 * (size_t)id);
    if (!off) return 0;
    if (off < 4 || off >= tsize) bad();
    return t + off;
  }
  template <typename T> T scalar(size_t t, int id, T def) const {
    const size_t p = field(t, id);
    if (!p) return def;
    const uint16_t tsize = rd<uint16_t>((size_t)((int64_t)t - rd<int32_t>(t)) + 2);
    if (p - t + sizeof(T) > tsize) bad();
    return rd<T>(p);
  }
  size_t indirect(size_t t, int id) const { const size_t p = field(t, id); return p ? follow(p) : 0; }
  // a vector's element count, after checking that `elem`-byte elements fit behind it
  uint32_t vec_len(size_t v, size_t elem) const {
    const uint32_t n = rd<uint32_t>(v);
    if ((len - v - 4) / elem < n) bad();
    return n;
  }
  std::string str(size_t t, int id) const {
    const size_t s = indirect(t, id);
    if (!s) return "";
    const uint32_t n = vec_len(s, 1);
    return std::string((const char*)base + s + 4, n);
  }
};

// ------------------------------------------------------------------------------------------------------- type <-> format
enum TypeTag : uint8_t { TY_Int = 2, TY_FloatingPoint = 3, TY_Utf8 = 5, TY_Bool = 6, TY_Decimal = 7, TY_Date = 8, TY_Time = 9,
                         TY_Timestamp = 10, TY_FixedSizeBinary = 15, TY_Duration = 18 };

int time_unit(char c) { return c == 's' ? 0 : c == 'm' ? 1 : c == 'u' ? 2 : 3; }
char unit_char(int u) { return "smun"[u & 3]; }

uint32_t write_type(FlatWriter& w, const std::string& f, uint8_t* tag) {
  const uint32_t start = w.mark();
  auto int_type = [&](int bits, bool sign) { w.start_table(); w.scalar<int32_t>(0, bits); w.scalar<uint8_t>(1, sign ? 1 : 0); *tag = TY_Int; return w.end_table(start); };
  auto fp = [&](int16_t prec) { w.start_table(); w.scalar<int16_t>(0, prec); *tag = TY_FloatingPoint; return w.end_table(start); };
  if (f == "b") { w.start_table(); *tag = TY_Bool; return w.end_table(start); }
  if (f == "u") { w.start_table(); *tag = TY_Utf8; return w.end_table(start); }
  if (f == "c") return int_type(8, true);   if (f == "C") return int_type(8, false);
  if (f == "s") return int_type(16, true);  if (f == "S") return int_type(16, false);
  if (f == "i") return int_type(32, true);  if (f == "I") return int_type(32, false);
  if (f == "l") return int_type(64, true);  if (f == "L") return int_type(64, false);
  if (f == "e") return fp(0); if (f == "f") return fp(1); if (f == "g") return fp(2);
  if (f == "tdD" || f == "tdm") { w.start_table(); w.scalar<int16_t>(0, f == "tdD" ? 0 : 1); *tag = TY_Date; return w.end_table(start); }
  if (f.size() == 3 && f[0] == 't' && f[1] == 't') {
    w.start_table(); w.scalar<int16_t>(0, (int16_t)time_unit(f[2])); w.scalar<int32_t>(1, (f[2] == 's' || f[2] == 'm') ? 32 : 64); *tag = TY_Time; return w.end_table(start);
  }
  if (f.size() >= 4 && f[0] == 't' && f[1] == 's' && f[3] == ':') {
    const std::string tz = f.substr(4);
    const uint32_t tzs = tz.empty() ? 0 : w.string(tz);
    const uint32_t st = w.mark();
    w.start_table(); w.scalar<int16_t>(0, (int16_t)time_unit(f[2])); w.ref(1, tzs); *tag = TY_Timestamp; return w.end_table(st);
  }
  if (f.size() == 3 && f[0] == 't' && f[1] == 'D') { w.start_table(); w.scalar<int16_t>(0, (int16_t)time_unit(f[2])); *tag = TY_Duration; return w.end_table(start); }
  if (f.rfind("d:", 0) == 0) {
    int p = 0, s = 0, bw = 128;
    if (sscanf(f.c_str(), "d:%d,%d,%d", &p, &s, &bw) < 2) throw ChqError{CHQ_ERR_NOT_SUPPORTED, "decimal format '" + f + "'"};
    w.start_table(); w.scalar<int32_t>(0, p); w.scalar<int32_t>(1, s); w.scalar<int32_t>(2, bw); *tag = TY_Decimal; return w.end_table(start);
  }
  if (f.rfind("w:", 0) == 0) { w.start_table(); w.scalar<int32_t>(0, atoi(f.c_str() + 2)); *tag = TY_FixedSizeBinary; return w.end_table(start); }
  throw ChqError{CHQ_ERR_NOT_SUPPORTED, "Arrow type with format '" + f + "' cannot be written as Arrow IPC by this build"};
}

// Type tables off the wire: a value the format does not define is refused (INVALID_ARGUMENT), never mapped onto a
// neighbouring type's width; a legal type outside this build's scope is NOT_SUPPORTED and named.
std::string read_type(const FlatReader& r, uint8_t tag, size_t t) {
  auto invalid = [](const std::string& what) -> ChqError { return ChqError{CHQ_ERR_ARROW_INVALID_ARGUMENT, "Arrow IPC type table: " + what}; };
  auto unit = [&](int id, int16_t def, const char* of) {
    const int u = r.scalar<int16_t>(t, id, def);
    if (u < 0 || u > 3) throw invalid(std::string(of) + " unit " + std::to_string(u));
    return unit_char(u);
  };
  switch (tag) {
    case TY_Bool: return "b";
    case TY_Utf8: return "u";
    case TY_Int: {
      const int bits = r.scalar<int32_t>(t, 0, 0); const bool sign = r.scalar<uint8_t>(t, 1, 0) != 0;
      switch (bits) { case 8: return sign ? "c" : "C"; case 16: return sign ? "s" : "S"; case 32: return sign ? "i" : "I"; case 64: return sign ? "l" : "L"; default: break; }
      throw invalid("Int bitWidth " + std::to_string(bits));
    }
    case TY_FloatingPoint: {
      const int p = r.scalar<int16_t>(t, 0, 0);
      if (p < 0 || p > 2) throw invalid("FloatingPoint precision " + std::to_string(p));
      return p == 0 ? "e" : p == 1 ? "f" : "g";
    }
    case TY_Date: {
      const int u = r.scalar<int16_t>(t, 0, 1);
      if (u != 0 && u != 1) throw invalid("Date unit " + std::to_string(u));
      return u == 0 ? "tdD" : "tdm";
    }
    case TY_Time: {
      const char u = unit(0, 1, "Time");
      const int bits = r.scalar<int32_t>(t, 1, 32);
      if (bits != ((u == 's' || u == 'm') ? 32 : 64)) throw invalid(std::string("Time unit '") + u + "' with bitWidth " + std::to_string(bits));
      return std::string("tt") + u;
    }
    case TY_Timestamp: return std::string("ts") + unit(0, 0, "Timestamp") + ":" + r.str(t, 1);
    case TY_Duration: return std::string("tD") + unit(0, 1, "Duration");
    case TY_Decimal: {
      const int p = r.scalar<int32_t>(t, 0, 0), s = r.scalar<int32_t>(t, 1, 0), bw = r.scalar<int32_t>(t, 2, 128);
      if (bw == 32 || bw == 64 || bw == 256)
        throw ChqError{CHQ_ERR_NOT_SUPPORTED, "Arrow IPC type Decimal" + std::to_string(bw) + " is outside this build's scope"};
      if (bw != 128) throw invalid("Decimal bitWidth " + std::to_string(bw));
      if (p < 1 || p > 38) throw invalid("Decimal128 precision " + std::to_string(p));
      return "d:" + std::to_string(p) + "," + std::to_string(s);
    }
    case TY_FixedSizeBinary: {
      const int w = r.scalar<int32_t>(t, 0, 0);
      if (w < 0) throw invalid("FixedSizeBinary byteWidth " + std::to_string(w));
      if (w == 0) throw ChqError{CHQ_ERR_NOT_SUPPORTED, "Arrow IPC type FixedSizeBinary(0) is outside this build's scope"};
      return "w:" + std::to_string(w);
    }
    default: break;
  }
  static const char* const kNames[] = {"NONE", "Null", "Int", "FloatingPoint", "Binary", "Utf8", "Bool", "Decimal", "Date", "Time", "Timestamp",
                                       "Interval", "List", "Struct", "Union", "FixedSizeBinary", "FixedSizeList", "Map", "Duration",
                                       "LargeBinary", "LargeUtf8", "LargeList", "RunEndEncoded", "BinaryView", "Utf8View", "ListView", "LargeListView"};
  if (tag == 0) throw invalid("field without a type");
  const std::string name = tag < sizeof(kNames) / sizeof(kNames[0]) ? kNames[tag] : "id " + std::to_string((int)tag);
  throw ChqError{CHQ_ERR_NOT_SUPPORTED, "Arrow IPC type " + name + " is outside this build's scope"};
}

void append_message(std::vector<uint8_t>& out, const std::vector<uint8_t>& fb) {   // continuation, size (padded to 8), flatbuffer
  const uint32_t cont = 0xFFFFFFFFu;
  const int32_t padded = (int32_t)((fb.size() + 7) / 8 * 8);
  const size_t at = out.size();
  out.resize(at + 8 + (size_t)padded, 0);
  memcpy(&out[at], &cont, 4); memcpy(&out[at + 4], &padded, 4);
  memcpy(&out[at + 8], fb.data(), fb.size());
}

constexpr int64_t kBodyAlign = 64;   // what arrow-rs and Arrow C++ writers use; the format asks for 8
int64_t align_up(int64_t v) { return (v + kBodyAlign - 1) / kBodyAlign * kBodyAlign; }

}  // namespace

// =====================================================================================================================
// encode
// =====================================================================================================================
IpcMessage record_to_ipc(Context& ctx, const Batch& dev, bool body_on_device) {
  const int64_t n = dev.nrows;
  if (!dev.on_device) throw ChqError{CHQ_ERR_INVALID_HANDLE, "record_to_ipc expects a device-resident batch"};
  // ---- layout: FieldNodes and Buffers in schema order, every buffer 64-byte aligned -------------------------------------
  struct Piece { int col; int kind; int64_t offset, length; };   // kind: 0 validity, 1 values / bitmap / offsets, 2 utf8 data
  std::vector<Piece> pieces;
  std::vector<std::pair<int64_t, int64_t>> nodes, buffers;
  std::vector<int64_t> null_counts(dev.cols.size(), 0);
  std::vector<std::pair<int32_t, int32_t>> utf8_ends(dev.cols.size(), {0, 0});
  // null counts the producer left unknown (-1) and the Utf8 byte ranges: small read-backs, one synchronisation
  {
    bool any = false;
    std::vector<BufferPtr> counters(dev.cols.size());
    std::vector<unsigned long long> host_counts(dev.cols.size(), 0);
    for (size_t c = 0; c < dev.cols.size(); ++c) {
      const Column& col = dev.cols[c];
      if (col.validity && col.null_count < 0 && n > 0) {
        counters[c] = make_device_buffer(16, ctx.device);
        check_hip(hipMemsetAsync(counters[c]->ptr, 0, 8, ctx.stream), "memset");
        check_hip(launch_count_bits(col.validity, col.offset, n, (unsigned long long*)counters[c]->ptr, ctx.stream), "launch count_bits_kernel");
        check_hip(hipMemcpyAsync(&host_counts[c], counters[c]->ptr, 8, hipMemcpyDeviceToHost, ctx.stream), "read back");
        any = true;
      }
      if (col.type == T_UTF8 && n > 0 && col.values) {
        const int32_t* offs = (const int32_t*)col.values0();
        check_hip(hipMemcpyAsync(&utf8_ends[c].first, offs, 4, hipMemcpyDeviceToHost, ctx.stream), "read offsets");
        check_hip(hipMemcpyAsync(&utf8_ends[c].second, offs + n, 4, hipMemcpyDeviceToHost, ctx.stream), "read offsets");
        any = true;
      }
    }
    if (any) check_hip(hipStreamSynchronize(ctx.stream), "hipStreamSynchronize");
    for (size_t c = 0; c < dev.cols.size(); ++c) {
      const Column& col = dev.cols[c];
      if (!col.validity) null_counts[c] = 0;
      else if (col.null_count >= 0) null_counts[c] = col.null_count;
      else null_counts[c] = n - (int64_t)host_counts[c];
    }
  }
  int64_t at = 0;
  for (size_t c = 0; c < dev.cols.size(); ++c) {
    const Column& col = dev.cols[c];
    nodes.push_back({n, null_counts[c]});
    auto add = [&](int kind, int64_t len) {
      buffers.push_back({at, len});
      if (len > 0) pieces.push_back({(int)c, kind, at, len});
      at = align_up(at + len);
    };
    add(0, null_counts[c] > 0 ? (n + 7) / 8 : 0);
    if (col.type == T_BOOL) add(1, (n + 7) / 8);
    else if (col.type == T_UTF8) { add(1, (n + 1) * 4); add(2, (int64_t)utf8_ends[c].second - utf8_ends[c].first); }
    else add(1, n * col.width);
  }
  const int64_t body_len = at;

  // ---- metadata --------------------------------------------------------------------------------------------------------
  std::vector<uint8_t> header;
  {
    FlatWriter w;
    std::vector<uint32_t> fields;
    for (const Column& col : dev.cols) {
      uint8_t tag = 0;
      const uint32_t type = write_type(w, col.format, &tag);
      const uint32_t name = w.string(col.name);
      const uint32_t children = w.offset_vector({});
      const uint32_t start = w.mark();
      w.start_table();
      w.ref(0, name); w.scalar<uint8_t>(1, col.nullable ? 1 : 0); w.scalar<uint8_t>(2, tag); w.ref(3, type); w.ref(5, children);
      fields.push_back(w.end_table(start));
    }
    const uint32_t fvec = w.offset_vector(fields);
    uint32_t start = w.mark();
    w.start_table(); w.scalar<int16_t>(0, 0); w.ref(1, fvec);
    const uint32_t schema = w.end_table(start);
    start = w.mark();
    w.start_table(); w.scalar<int16_t>(0, 4 /* V5 */); w.scalar<uint8_t>(1, 1 /* Schema */); w.ref(2, schema); w.scalar<int64_t>(3, 0);
    append_message(header, w.finish(w.end_table(start)));
  }
  {
    FlatWriter w;
    const uint32_t bvec = w.pair_vector(buffers);
    const uint32_t nvec = w.pair_vector(nodes);
    uint32_t start = w.mark();
    w.start_table(); w.scalar<int64_t>(0, n); w.ref(1, nvec); w.ref(2, bvec);
    const uint32_t rb = w.end_table(start);
    start = w.mark();
    w.start_table(); w.scalar<int16_t>(0, 4); w.scalar<uint8_t>(1, 3 /* RecordBatch */); w.ref(2, rb); w.scalar<int64_t>(3, body_len);
    append_message(header, w.finish(w.end_table(start)));
  }

  // ---- body: one HBM allocation, every piece placed by a device copy or a small kernel ------------------------------------
  BufferPtr body = make_device_buffer((size_t)body_len + 64, ctx.device);
  uint8_t* bp = (uint8_t*)body->ptr;
  if (body_len > 0) check_hip(hipMemsetAsync(bp, 0, (size_t)body_len, ctx.stream), "memset body");   // padding bytes are zero
  for (const Piece& pc : pieces) {
    const Column& col = dev.cols[(size_t)pc.col];
    uint8_t* dst = bp + pc.offset;
    const bool bitmap = pc.kind == 0 || (pc.kind == 1 && col.type == T_BOOL);
    if (bitmap) {
      const uint8_t* src = pc.kind == 0 ? col.validity : col.values;
      if ((col.offset & 7) == 0) check_hip(hipMemcpyAsync(dst, src + (col.offset >> 3), (size_t)pc.length, hipMemcpyDeviceToDevice, ctx.stream), "copy bitmap");
      else check_hip(launch_bit_shift_copy(src, col.offset, n, (uint32_t*)dst, ctx.stream), "launch bit_shift_copy_kernel");
    } else if (pc.kind == 1 && col.type == T_UTF8) {
      const int32_t* offs = (const int32_t*)col.values0();
      if (utf8_ends[(size_t)pc.col].first == 0) check_hip(hipMemcpyAsync(dst, offs, (size_t)pc.length, hipMemcpyDeviceToDevice, ctx.stream), "copy offsets");
      else check_hip(launch_rebase_offsets(offs, (int32_t*)dst, n + 1, ctx.stream), "launch rebase_offsets_kernel");
    } else if (pc.kind == 2) {
      check_hip(hipMemcpyAsync(dst, col.data + utf8_ends[(size_t)pc.col].first, (size_t)pc.length, hipMemcpyDeviceToDevice, ctx.stream), "copy string bytes");
    } else {
      check_hip(hipMemcpyAsync(dst, col.values0(), (size_t)pc.length, hipMemcpyDeviceToDevice, ctx.stream), "copy values");
    }
  }
  IpcMessage msg;
  msg.header = std::move(header);
  msg.body_len = body_len;
  if (body_on_device) {
    msg.body = body; msg.body_on_device = true;
  } else {
    BufferPtr host = make_host_buffer((size_t)body_len + 64);
    if (body_len > 0) check_hip(hipMemcpyAsync(host->ptr, bp, (size_t)body_len, hipMemcpyDeviceToHost, ctx.stream), "download body");
    msg.body = host; msg.body_on_device = false;
    msg.keep = body;   // until the copy below has completed
  }
  check_hip(hipStreamSynchronize(ctx.stream), "hipStreamSynchronize");
  msg.keep.reset();
  return msg;
}

// =====================================================================================================================
// decode
// =====================================================================================================================
namespace {
struct FieldInfo { std::string name, format; bool nullable = false; DType type = T_BOOL; int width = 0; };
struct ParsedStream {
  std::vector<FieldInfo> fields;
  int64_t n = 0, body_len = 0;
  std::vector<std::pair<int64_t, int64_t>> nodes, buffers;
  int64_t body_at = -1;       // position of the body inside the stream (right behind the batch message's metadata)
  bool header_only = false;   // the stream ends with the batch message's metadata: the body travels separately
};

[[noreturn]] void invalid_stream(const std::string& what) { throw ChqError{CHQ_ERR_ARROW_INVALID_ARGUMENT, what}; }

int64_t bitmap_bytes(int64_t n) { return n / 8 + (n % 8 != 0); }

// Everything the METADATA claims is checked here, on the host, before a byte of the body is copied or an allocation is sized
// by it: framing, the flatbuffers, type tables, row count, null counts and every (offset, length) against bodyLength.  Sizes
// from the wire are compared by subtraction / division only -- sums and products of forged 64-bit values wrap.
// `separate_body`: the caller passes the body on its own, so `stream` holds metadata only.
ParsedStream parse_stream(const uint8_t* stream, int64_t stream_len, bool separate_body) {
  if (!stream || stream_len < 8) invalid_stream("empty Arrow IPC stream");
  ParsedStream ps;
  bool have_schema = false, have_batch = false;
  int64_t at = 0;
  while (stream_len - at >= 4) {
    uint32_t first; memcpy(&first, stream + at, 4);
    int32_t msize;
    if (first == 0xFFFFFFFFu) {
      if (stream_len - at < 8) invalid_stream("truncated Arrow IPC message");
      memcpy(&msize, stream + at + 4, 4); at += 8;
    } else { msize = (int32_t)first; at += 4; }   // pre-0.15 framing without the continuation marker
    if (msize == 0) break;   // end of stream
    if (msize < 0 || msize > stream_len - at) invalid_stream("truncated Arrow IPC message");
    FlatReader r{stream + at, (size_t)msize};
    const size_t m = r.root();
    const uint8_t htype = r.scalar<uint8_t>(m, 1, 0);
    const size_t h = r.indirect(m, 2);
    const int64_t blen = r.scalar<int64_t>(m, 3, 0);
    at += msize;
    if (blen < 0) invalid_stream("Arrow IPC message with a negative bodyLength");
    if (htype == 1 && h) {   // Schema
      if (have_schema) invalid_stream("Arrow IPC stream with a second schema");
      if (r.scalar<int16_t>(h, 0, 0) != 0) throw ChqError{CHQ_ERR_NOT_SUPPORTED, "big-endian Arrow IPC streams are not supported"};
      const size_t fv = r.indirect(h, 1);
      const uint32_t nf = fv ? r.vec_len(fv, 4) : 0;
      for (uint32_t i = 0; i < nf; ++i) {
        const size_t f = r.follow(fv + 4 + 4 * (size_t)i);
        if (r.field(f, 4)) throw ChqError{CHQ_ERR_NOT_SUPPORTED, "dictionary-encoded fields are outside this build's scope"};
        const size_t ch = r.indirect(f, 5);
        if (ch && r.vec_len(ch, 4) != 0) throw ChqError{CHQ_ERR_NOT_SUPPORTED, "nested Arrow types are outside this build's scope"};
        FieldInfo fi;
        fi.name = r.str(f, 0); fi.nullable = r.scalar<uint8_t>(f, 1, 0) != 0;
        const size_t ty = r.indirect(f, 3);
        if (!ty) r.bad();
        fi.format = read_type(r, r.scalar<uint8_t>(f, 2, 0), ty);
        parse_arrow_format(fi.format.c_str(), &fi.type, &fi.width, true);   // the C-data format parser knows type and width; the decode only places bytes
        ps.fields.push_back(std::move(fi));
      }
      have_schema = true;
    } else if (htype == 3 && h) {   // RecordBatch
      if (!have_schema) invalid_stream("Arrow IPC record batch before its schema");
      // the reference refuses a second batch too (ExchangeRequestsError::ReceivedMultipleRecordBatches, exchange.rs:259-266)
      if (have_batch) invalid_stream("Arrow IPC stream with more than one record batch");
      if (const size_t comp = r.indirect(h, 3)) {
        const int codec = r.scalar<int8_t>(comp, 0, 0);
        throw ChqError{CHQ_ERR_NOT_SUPPORTED, std::string("compressed Arrow IPC bodies (") + (codec == 0 ? "LZ4_FRAME" : codec == 1 ? "ZSTD" : "unknown codec") +
                                                  ") are outside this build's scope"};
      }
      ps.n = r.scalar<int64_t>(h, 0, 0);
      auto pairs = [&](int id, std::vector<std::pair<int64_t, int64_t>>& out) {
        const size_t v = r.indirect(h, id);
        const uint32_t k = v ? r.vec_len(v, 16) : 0;
        for (uint32_t i = 0; i < k; ++i) out.push_back({r.rd<int64_t>(v + 4 + 16 * (size_t)i), r.rd<int64_t>(v + 4 + 16 * (size_t)i + 8)});
      };
      pairs(1, ps.nodes); pairs(2, ps.buffers);
      ps.body_len = blen;
      ps.body_at = at;
      have_batch = true;
      if (!separate_body) {
        if (at == stream_len && blen > 0) ps.header_only = true;
        else if (blen > stream_len - at) invalid_stream("Arrow IPC body is shorter than its metadata says");
        else at += blen;
      }
    } else if (htype == 2) {
      throw ChqError{CHQ_ERR_NOT_SUPPORTED, "dictionary batches are outside this build's scope"};
    } else {   // a message kind we do not need: step over its body, which must lie inside the stream
      if (blen > stream_len - at) invalid_stream("truncated Arrow IPC message body");
      at += blen;
    }
  }
  if (!have_schema || !have_batch) invalid_stream("Arrow IPC stream without a schema and a record batch");
  const int64_t n = ps.n, body = ps.body_len;
  if (n < 0 || ps.nodes.size() != ps.fields.size()) invalid_stream("Arrow IPC record batch does not match its schema");
  size_t bi = 0;
  auto take = [&](int64_t need, const char* what) {
    if (bi >= ps.buffers.size()) invalid_stream("Arrow IPC record batch has too few buffers");
    const auto [off, len] = ps.buffers[bi++];
    if (off < 0 || len < 0 || off > body || len > body - off || len < need)
      invalid_stream(std::string("Arrow IPC buffer (") + what + ") outside the body or too short");
  };
  // a column of n rows needs n * width (n / 8, 4 (n + 1)) bytes of the body: n is bounded by division before it is multiplied
  auto rows_fit = [&](int64_t per_row_num, int64_t per_row_den, const FieldInfo& f) {
    if (n / per_row_den > body / per_row_num) invalid_stream("Arrow IPC record batch length " + std::to_string(n) + " exceeds what the body can hold for column '" + f.name + "'");
  };
  for (size_t c = 0; c < ps.fields.size(); ++c) {
    const FieldInfo& f = ps.fields[c];
    const auto [len, nulls] = ps.nodes[c];
    if (len != n) invalid_stream("Arrow IPC field node length differs from the batch length");
    if (nulls < 0 || nulls > n) invalid_stream("Arrow IPC field node null count " + std::to_string(nulls) + " outside [0, length]");
    if (f.type == T_BOOL) rows_fit(1, 8, f);
    else if (f.type == T_UTF8) rows_fit(4, 1, f);
    else rows_fit(f.width, 1, f);
    take(nulls > 0 ? bitmap_bytes(n) : 0, "validity");
    if (f.type == T_BOOL) take(bitmap_bytes(n), "bitmap");
    else if (f.type == T_UTF8) {
      take(n > 0 ? (n + 1) * 4 : 0, "offsets");   // zero rows: older writers emit an empty offsets buffer; arrow-rs and Arrow C++ accept it
      take(0, "string bytes");
    } else take(n * f.width, "values");
  }
  return ps;
}
}  // namespace

// host only: what a stream's metadata says (the CPU test tier checks the flatbuffer reader against pyarrow's writer)
std::string describe_ipc(const uint8_t* stream, int64_t stream_len) {
  const ParsedStream ps = parse_stream(stream, stream_len, false);
  std::string out = "rows " + std::to_string(ps.n) + " body " + std::to_string(ps.body_len) + " body_at " + std::to_string(ps.body_at) + "\n";
  for (size_t c = 0; c < ps.fields.size(); ++c)
    out += "field " + ps.fields[c].name + " " + ps.fields[c].format + " nullable=" + (ps.fields[c].nullable ? "1" : "0") +
           " nulls=" + std::to_string(ps.nodes[c].second) + "\n";
  for (auto& b : ps.buffers) out += "buffer " + std::to_string(b.first) + " " + std::to_string(b.second) + "\n";
  return out;
}

Batch record_from_ipc(Context& ctx, const uint8_t* stream, int64_t stream_len, const void* body, int64_t body_len,
                      bool body_on_device, bool out_on_device) {
  const ParsedStream ps = parse_stream(stream, stream_len, body != nullptr);   // every size below has been validated there
  const std::vector<FieldInfo>& fields = ps.fields;
  const int64_t n = ps.n, meta_body_len = ps.body_len;
  const std::vector<std::pair<int64_t, int64_t>>& nodes = ps.nodes;
  const std::vector<std::pair<int64_t, int64_t>>& buffers = ps.buffers;
  if (body ? body_len < meta_body_len : ps.header_only) throw ChqError{CHQ_ERR_ARROW_INVALID_ARGUMENT, "Arrow IPC body is shorter than its metadata says"};
  const void* src_body = body ? body : (const void*)(stream + ps.body_at);
  const bool src_on_device = body ? body_on_device : false;

  // ---- the body goes to its destination with ONE copy; the columns are views into it -------------------------------------
  BufferPtr owned = out_on_device ? make_device_buffer((size_t)meta_body_len + 64, ctx.device) : make_host_buffer((size_t)meta_body_len + 64);
  uint8_t* const base = (uint8_t*)owned->ptr;
  if (meta_body_len > 0) {
    if (!out_on_device && !src_on_device) memcpy(base, src_body, (size_t)meta_body_len);
    else {
      const hipMemcpyKind k = out_on_device ? (src_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice) : hipMemcpyDeviceToHost;
      check_hip(hipMemcpyAsync(base, src_body, (size_t)meta_body_len, k, ctx.stream), "move Arrow IPC body");
    }
  }
  Batch out;
  out.nrows = n; out.on_device = out_on_device; out.device_id = out_on_device ? ctx.device : -1;
  size_t bi = 0;
  struct Utf8Check { const int32_t* offs; int64_t data_len; };      // validated after the copy landed
  struct NullCheck { const uint8_t* validity; int64_t claimed; };   // the bitmap must hold exactly the nulls the node claims
  std::vector<Utf8Check> utf8_checks;
  std::vector<NullCheck> null_checks;
  const uint8_t* zero_offset = nullptr;   // one zero Int32 in the allocation's slack, for zero-row Utf8 columns without offsets
  for (size_t c = 0; c < fields.size(); ++c) {
    Column col;
    col.name = fields[c].name; col.format = fields[c].format; col.nullable = fields[c].nullable;
    col.type = fields[c].type; col.width = fields[c].width;
    col.length = n; col.offset = 0; col.null_count = nodes[c].second;
    // a validity buffer next to null_count 0 is dropped, as Arrow C++ and arrow-rs do: every row is valid
    const uint8_t* validity = base + buffers[bi++].first;
    col.validity = col.null_count > 0 ? validity : nullptr;
    if (col.validity) null_checks.push_back({col.validity, col.null_count});
    col.values = base + buffers[bi].first;
    if (col.type == T_UTF8) {
      if (buffers[bi].second < 4) {   // only legal with zero rows (parse_stream)
        if (!zero_offset) {
          zero_offset = base + (meta_body_len + 7) / 8 * 8;
          if (out_on_device) check_hip(hipMemsetAsync((void*)zero_offset, 0, 8, ctx.stream), "memset");
          else memset((void*)zero_offset, 0, 8);
        }
        col.values = zero_offset;
      }
      ++bi;
      col.data = base + buffers[bi].first;
      if (n > 0) utf8_checks.push_back({(const int32_t*)col.values, buffers[bi].second});
    }
    ++bi;
    col.owned.push_back(owned);
    out.cols.push_back(std::move(col));
  }
  // What only the BODY can tell is checked once it has landed.  A kernel must never follow offsets out of the data buffer:
  // EVERY offset is checked (0 <= off[i] <= off[i+1] <= data length).  A null count that contradicts its bitmap is refused:
  // consumers size outputs and pick kernels by it.  For a device result these are one small kernel per Utf8 column and per
  // column with nulls, and one read-back (flag word + counters) with the synchronisation that was needed anyway; for a host
  // result, plain loops.
  BufferPtr flags;
  std::vector<unsigned long long> results(1 + null_checks.size(), 0);   // [0] the offsets flag, then set bits per bitmap
  if (out_on_device && n > 0 && (!utf8_checks.empty() || !null_checks.empty())) {
    flags = make_device_buffer(results.size() * 8, ctx.device);
    unsigned long long* dev = (unsigned long long*)flags->ptr;
    check_hip(hipMemsetAsync(dev, 0, results.size() * 8, ctx.stream), "memset");
    for (auto& chk : utf8_checks)
      check_hip(launch_validate_offsets(chk.offs, n, chk.data_len, (uint32_t*)dev, ctx.stream), "launch validate_offsets_kernel");
    for (size_t k = 0; k < null_checks.size(); ++k)
      check_hip(launch_count_bits(null_checks[k].validity, 0, n, dev + 1 + k, ctx.stream), "launch count_bits_kernel");
    check_hip(hipMemcpyAsync(results.data(), dev, results.size() * 8, hipMemcpyDeviceToHost, ctx.stream), "read back");
  }
  check_hip(hipStreamSynchronize(ctx.stream), "hipStreamSynchronize");
  if (!out_on_device) {
    bool bad = false;
    for (auto& chk : utf8_checks)
      for (int64_t i = 0; i < n && !bad; ++i) bad |= chk.offs[i] < 0 || chk.offs[i + 1] < chk.offs[i] || (int64_t)chk.offs[i + 1] > chk.data_len;
    results[0] = bad;
    for (size_t k = 0; k < null_checks.size(); ++k) {
      const uint8_t* v = null_checks[k].validity;
      unsigned long long set = 0;
      for (int64_t i = 0; i < n / 8; ++i) set += (unsigned)__builtin_popcount(v[i]);
      if (n % 8) set += (unsigned)__builtin_popcount(v[n / 8] & ((1u << (n % 8)) - 1u));
      results[1 + k] = set;
    }
  }
  if ((uint32_t)results[0]) throw ChqError{CHQ_ERR_ARROW_INVALID_ARGUMENT, "Arrow IPC Utf8 offsets are not monotonic or point outside the data buffer"};
  for (size_t k = 0; k < null_checks.size(); ++k)
    if (n - (int64_t)results[1 + k] != null_checks[k].claimed)
      throw ChqError{CHQ_ERR_ARROW_INVALID_ARGUMENT, "Arrow IPC field node claims " + std::to_string(null_checks[k].claimed) + " nulls, its validity bitmap holds " +
                                                          std::to_string(n - (int64_t)results[1 + k])};
  return out;
}

}  // namespace chq
