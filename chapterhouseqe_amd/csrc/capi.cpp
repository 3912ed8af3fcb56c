// capi.cpp -- the extern "C" surface declared in include/chq.h, except the expression handles (capi_expr.cpp).
#include <algorithm>
#include <cstring>
#include <exception>
#include <new>

#include "engine.hpp"
#include "parquet.hpp"
#include "sort.hpp"
#include "aggregate.hpp"
#include "window.hpp"
#include "join.hpp"
#include "partition.hpp"

using namespace chq;

struct chq_ctx { Context c; };
struct chq_parquet { PqFile file; };

namespace {

chq_status status_of(const ChqError& e) { return e.code == CHQ_INTERNAL_PROGRAM_LIMIT ? CHQ_ERR_NOT_SUPPORTED : (chq_status)e.code; }

template <typename F>
chq_status guarded(chq_ctx* ctx, F&& f) {
  try {
    f();
    if (ctx) ctx->c.last_error.clear();
    return CHQ_OK;
  } catch (const ChqError& e) {
    if (ctx) ctx->c.last_error = e.msg;
    return status_of(e);
  } catch (const std::bad_alloc&) {
    if (ctx) ctx->c.last_error = "out of host memory";
    return CHQ_ERR_OUT_OF_MEMORY;
  } catch (const std::exception& e) {
    if (ctx) ctx->c.last_error = e.what();
    return CHQ_ERR_DEVICE;
  }
}

// ---- the frame of an entry that takes a context -----------------------------------------------------------------------------
// A null context returns before the caller's structs are touched.  Then `clear` makes the outputs read as released, and
// `body` -- the entry's checks in their documented order, then its work -- runs under `guarded`.
template <class Clear, class Body>
chq_status host_entry(chq_ctx* ctx, Clear&& clear, Body&& body) {
  if (!ctx) return CHQ_ERR_INVALID_HANDLE;
  clear();
  return guarded(ctx, body);
}
// the same with the context's GPU current: every entry that may touch the device
template <class Clear, class Body>
chq_status entry(chq_ctx* ctx, Clear&& clear, Body&& body) {
  return host_entry(ctx, clear, [&] { ctx->c.typed_stats = chq_call_stats{}; check_hip(hipSetDevice(ctx->c.device), "hipSetDevice"); body(); });
}
// context in, one record out
template <class Body>
chq_status record_entry(chq_ctx* ctx, ArrowDeviceArray* out, ArrowSchema* out_schema, Body&& body) {
  return entry(ctx, [&] { mark_released(out, out_schema); }, body);
}
// context in, outs[0..n) / out_schemas[0..n) out: every output or none
template <class Body>
chq_status records_entry(chq_ctx* ctx, int n, ArrowDeviceArray* outs, ArrowSchema* out_schemas, Body&& body) {
  return entry(ctx, [&] { for (int i = 0; i < n; ++i) mark_released(outs ? &outs[i] : nullptr, out_schemas ? &out_schemas[i] : nullptr); },
               [&] {
                 try {
                   body();
                 } catch (...) {   // no partial output
                   for (int i = 0; i < n; ++i) {
                     if (outs && outs[i].array.release) outs[i].array.release(&outs[i].array);
                     if (out_schemas && out_schemas[i].release) out_schemas[i].release(&out_schemas[i]);
                   }
                   throw;
                 }
               });
}

// ---- the checks the entries share -------------------------------------------------------------------------------------------
void require(const void* p, const char* what) { if (!p) throw ChqError{CHQ_ERR_INVALID_HANDLE, std::string("null ") + what}; }
[[noreturn]] void invalid(const std::string& msg) { throw ChqError{CHQ_ERR_ARROW_INVALID_ARGUMENT, msg}; }

void require_out(const ArrowDeviceArray* out, const ArrowSchema* out_schema) { require(out, "output array"); require(out_schema, "output schema"); }
void require_out_device(int out_device) {
  if (out_device != ARROW_DEVICE_ROCM && out_device != ARROW_DEVICE_CPU) invalid("out_device must be ARROW_DEVICE_CPU or ARROW_DEVICE_ROCM");
}
void require_records(int n, const ArrowDeviceArray* const* recs) {
  if (n <= 0) invalid("at least one record batch is needed");
  require(recs, "record array");
}
// `what`: "sort", "GROUP BY", "PARTITION BY", "ORDER BY", "partition", "join"
void require_keys(int n, const void* keys, const char* what) {
  if (n < 0) invalid(std::string("negative ") + what + " key count");
  if (n > 0 && !keys) throw ChqError{CHQ_ERR_INVALID_HANDLE, std::string("null ") + what + " keys"};
}
void require_each(int n, const ArrowDeviceArray* const* recs, const char* what) { for (int i = 0; i < n; ++i) require(recs[i], what); }

// the *_record entries, handed no record (before the *_records call, which takes the record in an array of one)
chq_status null_record(chq_ctx* ctx, ArrowDeviceArray* out, ArrowSchema* out_schema) {
  return host_entry(ctx, [&] { mark_released(out, out_schema); }, [] { require(nullptr, "record"); });
}

// the C arrays of a call as the engine takes them; a null element is CHQ_ERR_INVALID_HANDLE "null <what>"
std::vector<const Expr*> expr_args(const chq_expr* const* keys, int n, const char* what) {
  std::vector<const Expr*> args((size_t)n);
  for (int k = 0; k < n; ++k) {
    require(keys[k], what);
    args[(size_t)k] = &keys[k]->e;
  }
  return args;
}

std::vector<SortKeyArg> sort_key_args(const chq_sort_key* keys, int n, const char* what) {
  std::vector<SortKeyArg> args((size_t)n);
  for (int k = 0; k < n; ++k) {
    require(keys[k].column, what);
    args[(size_t)k].column = &keys[k].column->e;
    args[(size_t)k].descending = keys[k].descending != 0;
    args[(size_t)k].nulls_first = keys[k].nulls_first != 0;
  }
  return args;
}

std::vector<chq_select_item> select_items(const chq_select_item* fields, int n_fields) {
  if (n_fields > 0) require(fields, "select items");
  return std::vector<chq_select_item>(fields, fields + (n_fields > 0 ? n_fields : 0));
}

// ---- in and out -------------------------------------------------------------------------------------------------------------
// the batches of one group: every record is required before the first is imported
std::vector<Batch> import_records(int n, const ArrowDeviceArray* const* recs, const ArrowSchema* schema, const char* what = "record") {
  require_each(n, recs, what);
  std::vector<Batch> in((size_t)n);
  for_each_parallel(n, [&](int i) { in[(size_t)i] = import_batch(recs[i], schema); });
  return in;
}

// a batch in HBM (staged when it came from the host) and its columns as the planner sees them
struct DeviceBatch { Batch dev; std::vector<PlanColumn> pcols; };
DeviceBatch device_batch(chq_ctx* ctx, const Batch& in, const chq_table_aliases* aliases) {
  DeviceBatch d;
  d.dev = to_device(ctx->c, in);
  d.pcols = plan_columns(d.dev, aliases);
  return d;
}
DeviceBatch device_batch(chq_ctx* ctx, const ArrowDeviceArray* rec, const ArrowSchema* schema, const chq_table_aliases* aliases) {
  return device_batch(ctx, import_batch(rec, schema), aliases);
}

void finish(Context& c, Batch&& result_dev, int out_device, ArrowDeviceArray* out, ArrowSchema* out_schema) {
  require_out_device(out_device);
  if (out_device == ARROW_DEVICE_ROCM) export_batch(std::move(result_dev), ARROW_DEVICE_ROCM, out, out_schema);
  else { Batch h = to_host(c, result_dev); export_batch(std::move(h), ARROW_DEVICE_CPU, out, out_schema); }
}

// The phases of a blocking operator's call -- import, run, export -- with the marks CHQ_TIMING=1 prints between them.
template <class Import, class Run, class Export>
void phased(const char* entry_name, const char* phase, Import&& import, Run&& run, Export&& export_result) {
  PhaseTimer pt(entry_name);
  auto in = import();
  pt.mark("import");
  auto res = run(in);
  pt.mark(phase);
  export_result(res);
  pt.mark("export");
}
// one group in, one batch out (sort, aggregate, window)
template <class Run>
void blocking_call(chq_ctx* ctx, const char* entry_name, const char* phase, int n_records, const ArrowDeviceArray* const* recs,
                   const ArrowSchema* schema, int out_device, ArrowDeviceArray* out, ArrowSchema* out_schema, Run&& run) {
  phased(entry_name, phase, [&] { return import_records(n_records, recs, schema); }, run,
         [&](Batch& res) { finish(ctx->c, std::move(res), out_device, out, out_schema); });
}

// ---- text results (the entries without a context) ---------------------------------------------------------------------------
void copy_text(char* buf, size_t buf_len, const std::string& text) {
  if (buf && buf_len) { const size_t n = std::min(buf_len - 1, text.size()); memcpy(buf, text.data(), n); buf[n] = 0; }
}
// `buf` receives what `f` returns, or the message of what it throws; `other`: the status of an exception that is no ChqError
template <class F>
chq_status text_result(char* buf, size_t buf_len, chq_status other, F&& f) {
  std::string text;
  chq_status st = CHQ_OK;
  try {
    text = f();
  } catch (const ChqError& e) {
    st = status_of(e); text = e.msg;
  } catch (const std::exception& e) {
    st = other; text = e.what();
  }
  copy_text(buf, buf_len, text);
  return st;
}

// ---- Parquet handles and images ---------------------------------------------------------------------------------------------
// *out = a handle on the file `open` returns; `err`: the message when it throws
template <class Open>
chq_status open_parquet(chq_parquet** out, char* err, size_t err_len, Open&& open) {
  if (!out) return CHQ_ERR_ARROW_INVALID_ARGUMENT;
  *out = nullptr;
  return text_result(err, err_len, CHQ_ERR_ARROW_INVALID_ARGUMENT, [&] {
    std::unique_ptr<chq_parquet> h(new chq_parquet());
    h->file = open();
    *out = h.release();
    return std::string();
  });
}

struct ParquetImageHolder { chq::ParquetImage img; };
void clear_image(chq_parquet_image* m) { m->data = nullptr; m->len = 0; m->release = nullptr; m->private_data = nullptr; }
void release_parquet_image(chq_parquet_image* m) {
  if (!m || !m->release) return;
  delete (ParquetImageHolder*)m->private_data;
  clear_image(m);
}
// context in, one Parquet image out: `write` returns the image once the entry's own checks have passed
template <class Write>
chq_status image_entry(chq_ctx* ctx, chq_parquet_image* out, Write&& write) {
  return entry(ctx, [&] { if (out) clear_image(out); }, [&] {
    require(out, "output image");
    std::unique_ptr<ParquetImageHolder> h(new ParquetImageHolder());
    h->img = write();
    out->data = (const uint8_t*)h->img.bytes->ptr; out->len = h->img.len;
    out->release = release_parquet_image; out->private_data = h.release();
  });
}

}  // namespace

extern "C" {

int chq_abi_version(void) { return CHQ_ABI_VERSION; }

const char* chq_status_name(chq_status s) {
  switch (s) {
    case CHQ_OK: return "Ok";
    case CHQ_ERR_VALUE_TYPE_NOT_IMPLEMENTED: return "ComputeValueError::ValueTypeNotImplemented";
    case CHQ_ERR_EXPRESSION_TYPE_NOT_IMPLEMENTED: return "ComputeValueError::ExpressionTypeNotImplemented";
    case CHQ_ERR_BINARY_OPERATOR_NOT_IMPLEMENTED: return "ComputeValueError::BinaryOperatorNotImplemented";
    case CHQ_ERR_BINARY_OPERATION_CAST_FAILED: return "ComputeValueError::BinaryOperatinCastFailed";
    case CHQ_ERR_FAILED_TO_PARSE_AS_AN_INTEGER: return "ComputeValueError::FailedToParseAsAnInteger";
    case CHQ_ERR_FAILED_TO_PARSE_AS_A_FLOAT: return "ComputeValueError::FailedToParseAsAFloat";
    case CHQ_ERR_COLUMN_NOT_FOUND: return "ComputeValueError::ColumnNotFound";
    case CHQ_ERR_IDENTIFIER_NOT_FOUND: return "ComputeValueError::IdentifierNotFound";
    case CHQ_ERR_UNSUPPORTED_TYPE_COERSION: return "ComputeValueError::UnsupportedTypeCoersionForOperationBetweenTypes";
    case CHQ_ERR_CAST_TO_BOOLEAN_ARRAY_FAILED: return "FilterRecordError::CastToBooleanArrayFailedForArrayType";
    case CHQ_ERR_PROJECT_NOT_IMPLEMENTED: return "ProjectRecordError::NotImplemented";
    case CHQ_ERR_ARROW_ARITHMETIC_OVERFLOW: return "ArrowError::ArithmeticOverflow";
    case CHQ_ERR_ARROW_DIVIDE_BY_ZERO: return "ArrowError::DivideByZero";
    case CHQ_ERR_ARROW_INVALID_ARGUMENT: return "ArrowError::InvalidArgumentError";
    case CHQ_ERR_ARROW_COMPUTE: return "ArrowError::ComputeError";
    case CHQ_ERR_ARROW_CAST: return "ArrowError::CastError";
    case CHQ_ERR_NOT_SUPPORTED: return "NotSupported";
    case CHQ_ERR_INVALID_HANDLE: return "InvalidHandle";
    case CHQ_ERR_DEVICE: return "DeviceError";
    case CHQ_ERR_OUT_OF_MEMORY: return "OutOfMemory";
  }
  return "Unknown";
}

chq_status chq_ctx_create(int device_id, void* hip_stream, chq_ctx** out) {
  if (!out) return CHQ_ERR_INVALID_HANDLE;
  *out = nullptr;
  chq_ctx* ctx = new (std::nothrow) chq_ctx();
  if (!ctx) return CHQ_ERR_OUT_OF_MEMORY;
  chq_status st = guarded(ctx, [&] {
    int n = 0;
    check_hip(hipGetDeviceCount(&n), "hipGetDeviceCount");
    if (n <= 0 || device_id < 0 || device_id >= n) throw ChqError{CHQ_ERR_DEVICE, "no usable GPU for device id " + std::to_string(device_id)};
    check_hip(hipSetDevice(device_id), "hipSetDevice");
    hipDeviceProp_t prop;
    check_hip(hipGetDeviceProperties(&prop, device_id), "hipGetDeviceProperties");
    ctx->c.device = device_id;
    ctx->c.num_cus = prop.multiProcessorCount;
    if (hip_stream == (void*)hipStreamLegacy) {
      // The legacy default stream has two spellings, hipStreamLegacy ((hipStream_t)1) and the null handle; the library
      // keeps the NULL one.  ROCm 7.2's hipEventRecord stores the handle it was given in the event (guarding its own use
      // with `handle <= 1`), and hipStreamWaitEvent on such an event checks that field only against NULL before
      // dereferencing it: an event recorded on hipStreamLegacy makes any later hipStreamWaitEvent read address 0x249
      // (DESIGN.md section 5.1).  Same stream, no special handle ever reaches an event.
      ctx->c.stream = nullptr; ctx->c.own_stream = false;
    } else if (hip_stream) { ctx->c.stream = (hipStream_t)hip_stream; ctx->c.own_stream = false; }
    else { check_hip(hipStreamCreateWithFlags(&ctx->c.stream, hipStreamNonBlocking), "hipStreamCreate"); ctx->c.own_stream = true; }
  });
  if (st != CHQ_OK) { delete ctx; return st; }
  *out = ctx;
  return CHQ_OK;
}

void chq_ctx_destroy(chq_ctx* ctx) { delete ctx; }
const char* chq_ctx_last_error(const chq_ctx* ctx) { return ctx ? ctx->c.last_error.c_str() : "null context"; }
void* chq_ctx_stream(const chq_ctx* ctx) { return ctx ? (void*)ctx->c.stream : nullptr; }
void chq_ctx_last_stats(const chq_ctx* ctx, chq_call_stats* out) {
  if (!ctx || !out) return;
  *out = ctx->c.stats;
  // (the temporal kernels of the call's expressions: counted apart, see Context::typed_stats)
  out->launches += ctx->c.typed_stats.launches;
  out->bytes_read_alg += ctx->c.typed_stats.bytes_read_alg;
  out->bytes_written_alg += ctx->c.typed_stats.bytes_written_alg;
  out->kernel_ns += ctx->c.typed_stats.kernel_ns;
}

chq_status chq_ctx_set_option(chq_ctx* ctx, const char* key, int64_t value) {
  if (!ctx || !key) return CHQ_ERR_INVALID_HANDLE;
  return guarded(ctx, [&] {
    std::string k(key);
    if (k == "tile_kind") { if (value < -1 || value > 2) throw ChqError{CHQ_ERR_ARROW_INVALID_ARGUMENT, "tile_kind must be -1..2"}; ctx->c.opt_tile_kind = value; }
    else if (k == "enable_minus") ctx->c.opt_enable_minus = value != 0;
    else if (k == "time_kernels") ctx->c.opt_time_kernels = value != 0;
    else if (k == "fold_utf8") ctx->c.opt_fold_utf8 = value != 0;
    else if (k == "group_fold") ctx->c.opt_group_fold = value != 0;
    else if (k == "group_bits") ctx->c.opt_group_bits = value != 0;
    else if (k == "uniform_utf8_rows") ctx->c.opt_uniform_utf8_rows = value < 0 ? 0 : value;
    else if (k == "snappy_blocks") { if (value < 0 || value > 3) throw ChqError{CHQ_ERR_ARROW_INVALID_ARGUMENT, "snappy_blocks is 0, 1, 2 or 3"}; ctx->c.opt_snappy_blocks = value; }
    else if (k == "parquet_page_rows") { if (value < 1) throw ChqError{CHQ_ERR_ARROW_INVALID_ARGUMENT, "parquet_page_rows must be positive"}; ctx->c.opt_parquet_page_rows = value; }
    else if (k == "large_host") ctx->c.opt_large_host = value != 0;
    else if (k == "large_host_chunk") { if (value < 0) throw ChqError{CHQ_ERR_ARROW_INVALID_ARGUMENT, "large_host_chunk must not be negative"}; ctx->c.opt_large_host_chunk = value; }
    else if (k == "large_host_rows") { if (value < 1) throw ChqError{CHQ_ERR_ARROW_INVALID_ARGUMENT, "large_host_rows must be positive"}; ctx->c.opt_large_host_rows = value; }
    else if (k == "stash") { if (value < -1 || value > MAX_STASH) throw ChqError{CHQ_ERR_ARROW_INVALID_ARGUMENT, "stash must be -1..2"}; ctx->c.opt_stash = value; }
    else if (k == "small_host") ctx->c.opt_small_host = value != 0;
    else if (k == "fuse") { if (value < 0 || value > 2) throw ChqError{CHQ_ERR_ARROW_INVALID_ARGUMENT, "fuse must be 0..2"}; ctx->c.opt_fuse = value; }
    else if (k == "grid_per_cu") ctx->c.opt_grid_per_cu = value;
    else if (k == "split_rows") ctx->c.opt_split_rows = value;
    else if (k == "group_mode") ctx->c.opt_group_mode = value;
    else if (k == "group_chunk_bytes") { if (value < 1 || value > (1ll << 30)) throw ChqError{CHQ_ERR_ARROW_INVALID_ARGUMENT, "group_chunk_bytes must be 1..2^30"}; ctx->c.opt_group_chunk_bytes = value; }
    else if (k == "trim_pool") { DevicePool::instance().trim(); HostPool::instance().trim(); }
    else if (k == "host_pool_bytes") HostPool::instance().set_limit((size_t)(value < 0 ? 0 : value));
    else throw ChqError{CHQ_ERR_ARROW_INVALID_ARGUMENT, "unknown option: " + k};
  });
}

// ---- the path -------------------------------------------------------------------------------------------
chq_status chq_filter_record(chq_ctx* ctx, const ArrowDeviceArray* rec, const ArrowSchema* schema,
                             const chq_table_aliases* table_aliases, const chq_expr* expr, int out_device,
                             ArrowDeviceArray* out, ArrowSchema* out_schema) {
  return record_entry(ctx, out, out_schema, [&] {
    require(expr, "expression"); require_out(out, out_schema);
    Batch in = import_batch(rec, schema);
    if (out_device == ARROW_DEVICE_CPU && !in.on_device) {   // the reference's calling pattern: small host batch in, host batch out
      Batch small;
      if (filter_record_small_host(ctx->c, in, table_aliases, expr->e, &small) ||
          filter_record_large_host(ctx->c, in, table_aliases, expr->e, &small)) {
        export_batch(std::move(small), ARROW_DEVICE_CPU, out, out_schema);
        return;
      }
    }
    DeviceBatch d = device_batch(ctx, in, table_aliases);
    Batch res = filter_record(ctx->c, d.dev, d.pcols, expr->e);
    finish(ctx->c, std::move(res), out_device, out, out_schema);
  });
}

chq_status chq_plan_describe(const ArrowSchema* schema, const chq_table_aliases* table_aliases, const chq_expr* expr,
                             int64_t n_rows, int enable_minus, char* buf, size_t buf_len) {
  return text_result(buf, buf_len, CHQ_ERR_DEVICE, [&] {
    require(expr, "expression");
    return describe_plan(schema, table_aliases, expr->e, n_rows, enable_minus != 0);
  });
}

chq_status chq_filter_records(chq_ctx* ctx, int n_records, const ArrowDeviceArray* const* recs, const ArrowSchema* schema,
                              const chq_table_aliases* table_aliases, const chq_expr* expr, int out_device,
                              ArrowDeviceArray* outs, ArrowSchema* out_schemas) {
  return records_entry(ctx, n_records, outs, out_schemas, [&] {
    require(expr, "expression");
    if (n_records < 0) invalid("negative record count");
    if (n_records == 0) return;
    require(recs, "record array"); require(outs, "output arrays"); require(out_schemas, "output schemas");
    require_out_device(out_device);
    PhaseTimer pt("chq_filter_records");
    GroupInput gi;   // (filled in place: gi.materialise refers to it)
    require_each(n_records, recs, "record");
    import_group(n_records, recs, schema, ctx->c.device, gi);
    pt.mark("import");
    GroupResult res = filter_records(ctx->c, gi, table_aliases, expr->e, out_device == ARROW_DEVICE_ROCM);
    pt.mark("filter");
    if (res.batches() != (size_t)n_records)
      throw ChqError{CHQ_ERR_DEVICE, "internal error: the group result covers " + std::to_string(res.batches()) + " of " + std::to_string(n_records) + " batches"};
    size_t at = 0;
    for (JoinedGroup& part : res.parts) {
      const size_t n = part.ends.size();
      export_group(std::move(part), out_device, outs + at, out_schemas + at);
      at += n;
    }
    if (res.parts.empty()) for_each_parallel(n_records, [&](int i) { export_batch(std::move(res.per_batch[(size_t)i]), out_device, &outs[i], &out_schemas[i]); });
    pt.mark("export");
  });
}

chq_status chq_filter_records_coalesced(chq_ctx* ctx, int n_records, const ArrowDeviceArray* const* recs, const ArrowSchema* schema,
                                        const chq_table_aliases* table_aliases, const chq_expr* expr, int out_device,
                                        ArrowDeviceArray* out, ArrowSchema* out_schema, int64_t* rows_per_record) {
  return record_entry(ctx, out, out_schema, [&] {
    require(expr, "expression"); require_out(out, out_schema);
    require_records(n_records, recs);
    require_out_device(out_device);
    PhaseTimer pt("chq_filter_records_coalesced");
    GroupInput gi;   // (filled in place: gi.materialise refers to it)
    require_each(n_records, recs, "record");
    import_group(n_records, recs, schema, ctx->c.device, gi);
    pt.mark("import");
    std::vector<int64_t> rows;
    Batch res = filter_records_coalesced(ctx->c, gi, table_aliases, expr->e, out_device == ARROW_DEVICE_ROCM, &rows);
    pt.mark("filter");
    if (rows.size() != (size_t)n_records)
      throw ChqError{CHQ_ERR_DEVICE, "internal error: the coalesced result covers " + std::to_string(rows.size()) + " of " + std::to_string(n_records) + " batches"};
    if (rows_per_record) for (int i = 0; i < n_records; ++i) rows_per_record[i] = rows[(size_t)i];
    export_batch(std::move(res), out_device, out, out_schema);
    pt.mark("export");
  });
}

// ---- ORDER BY (sort.cpp) ---------------------------------------------------------------------------------------------------
chq_status chq_sort_records(chq_ctx* ctx, int n_records, const ArrowDeviceArray* const* recs, const ArrowSchema* schema,
                            const chq_table_aliases* table_aliases, const chq_sort_key* keys, int n_keys, int64_t limit,
                            int out_device, ArrowDeviceArray* out, ArrowSchema* out_schema) {
  return record_entry(ctx, out, out_schema, [&] {
    require_out(out, out_schema);
    require_records(n_records, recs);
    require_keys(n_keys, keys, "sort");
    require_out_device(out_device);
    const std::vector<SortKeyArg> args = sort_key_args(keys, n_keys, "sort key column");
    blocking_call(ctx, "chq_sort_records", "sort", n_records, recs, schema, out_device, out, out_schema,
                  [&](std::vector<Batch>& in) { return sort_records(ctx->c, in, table_aliases, args, limit); });
  });
}

chq_status chq_sort_record(chq_ctx* ctx, const ArrowDeviceArray* rec, const ArrowSchema* schema, const chq_table_aliases* table_aliases,
                           const chq_sort_key* keys, int n_keys, int64_t limit, int out_device, ArrowDeviceArray* out,
                           ArrowSchema* out_schema) {
  const ArrowDeviceArray* recs[1] = {rec};
  if (!rec) return null_record(ctx, out, out_schema);
  return chq_sort_records(ctx, 1, recs, schema, table_aliases, keys, n_keys, limit, out_device, out, out_schema);
}

// ---- GROUP BY (aggregate.cpp) ------------------------------------------------------------------------------------------------
chq_status chq_aggregate_records(chq_ctx* ctx, int n_records, const ArrowDeviceArray* const* recs, const ArrowSchema* schema,
                                 const chq_table_aliases* table_aliases, const chq_expr* const* keys, int n_keys,
                                 const chq_agg_item* items, int n_items, int out_device, ArrowDeviceArray* out, ArrowSchema* out_schema) {
  return record_entry(ctx, out, out_schema, [&] {
    require_out(out, out_schema);
    require_records(n_records, recs);
    require_keys(n_keys, keys, "GROUP BY");
    if (n_items <= 0) invalid("GROUP BY needs at least one output item");
    require(items, "output items");
    require_out_device(out_device);
    const std::vector<const Expr*> key_args = expr_args(keys, n_keys, "GROUP BY key");
    std::vector<AggItemArg> item_args((size_t)n_items);
    for (int i = 0; i < n_items; ++i) {
      AggItemArg& a = item_args[(size_t)i];
      a.kind = items[i].kind; a.key_index = items[i].key_index;
      a.column = items[i].column ? &items[i].column->e : nullptr;
      require(items[i].name, "output column name");
      a.name = items[i].name;
    }
    blocking_call(ctx, "chq_aggregate_records", "aggregate", n_records, recs, schema, out_device, out, out_schema,
                  [&](std::vector<Batch>& in) { return aggregate_records(ctx->c, in, table_aliases, key_args, item_args); });
  });
}

chq_status chq_aggregate_record(chq_ctx* ctx, const ArrowDeviceArray* rec, const ArrowSchema* schema, const chq_table_aliases* table_aliases,
                                const chq_expr* const* keys, int n_keys, const chq_agg_item* items, int n_items, int out_device,
                                ArrowDeviceArray* out, ArrowSchema* out_schema) {
  const ArrowDeviceArray* recs[1] = {rec};
  if (!rec) return null_record(ctx, out, out_schema);
  return chq_aggregate_records(ctx, 1, recs, schema, table_aliases, keys, n_keys, items, n_items, out_device, out, out_schema);
}

// ---- window functions (window.cpp) -----------------------------------------------------------------------------------------
chq_status chq_window_records(chq_ctx* ctx, int n_records, const ArrowDeviceArray* const* recs, const ArrowSchema* schema,
                              const chq_table_aliases* table_aliases, const chq_expr* const* partition_by, int n_partition_by,
                              const chq_sort_key* order_by, int n_order_by, const chq_window_item* items, int n_items, int out_device,
                              ArrowDeviceArray* out, ArrowSchema* out_schema) {
  return record_entry(ctx, out, out_schema, [&] {
    require_out(out, out_schema);
    require_records(n_records, recs);
    require_keys(n_partition_by, partition_by, "PARTITION BY");
    require_keys(n_order_by, order_by, "ORDER BY");
    if (n_items <= 0) invalid("a window call needs at least one item");
    require(items, "window items");
    require_out_device(out_device);
    const std::vector<const Expr*> part_args = expr_args(partition_by, n_partition_by, "PARTITION BY key");
    const std::vector<SortKeyArg> order_args = sort_key_args(order_by, n_order_by, "ORDER BY key column");
    std::vector<WinItemArg> item_args((size_t)n_items);
    for (int i = 0; i < n_items; ++i) {
      WinItemArg& a = item_args[(size_t)i];
      a.kind = items[i].kind; a.frame = items[i].frame; a.offset = items[i].offset;
      a.column = items[i].column ? &items[i].column->e : nullptr;
      require(items[i].name, "output column name");
      a.name = items[i].name;
    }
    blocking_call(ctx, "chq_window_records", "window", n_records, recs, schema, out_device, out, out_schema,
                  [&](std::vector<Batch>& in) { return window_records(ctx->c, in, table_aliases, part_args, order_args, item_args); });
  });
}

chq_status chq_window_record(chq_ctx* ctx, const ArrowDeviceArray* rec, const ArrowSchema* schema, const chq_table_aliases* table_aliases,
                             const chq_expr* const* partition_by, int n_partition_by, const chq_sort_key* order_by, int n_order_by,
                             const chq_window_item* items, int n_items, int out_device, ArrowDeviceArray* out, ArrowSchema* out_schema) {
  const ArrowDeviceArray* recs[1] = {rec};
  if (!rec) return null_record(ctx, out, out_schema);
  return chq_window_records(ctx, 1, recs, schema, table_aliases, partition_by, n_partition_by, order_by, n_order_by, items, n_items, out_device,
                            out, out_schema);
}

// ---- JOIN (join.cpp) ---------------------------------------------------------------------------------------------------------
chq_status chq_join_records(chq_ctx* ctx, int n_left, const ArrowDeviceArray* const* left, const ArrowSchema* left_schema,
                            const chq_table_aliases* left_aliases, int n_right, const ArrowDeviceArray* const* right,
                            const ArrowSchema* right_schema, const chq_table_aliases* right_aliases, const chq_join_key* keys, int n_keys,
                            int out_device, ArrowDeviceArray* out, ArrowSchema* out_schema) {
  return chq_join_records_kind(ctx, n_left, left, left_schema, left_aliases, n_right, right, right_schema, right_aliases, keys, n_keys,
                               CHQ_JOIN_INNER, out_device, out, out_schema);
}

chq_status chq_join_records_kind(chq_ctx* ctx, int n_left, const ArrowDeviceArray* const* left, const ArrowSchema* left_schema,
                                 const chq_table_aliases* left_aliases, int n_right, const ArrowDeviceArray* const* right,
                                 const ArrowSchema* right_schema, const chq_table_aliases* right_aliases, const chq_join_key* keys, int n_keys,
                                 int kind, int out_device, ArrowDeviceArray* out, ArrowSchema* out_schema) {
  return record_entry(ctx, out, out_schema, [&] {
    require_out(out, out_schema);
    if (n_left <= 0 || n_right <= 0) invalid("at least one record batch per side is needed");
    require(left, "left record array"); require(right, "right record array");
    require(left_schema, "left schema"); require(right_schema, "right schema");
    if (kind < CHQ_JOIN_INNER || kind > CHQ_JOIN_LEFT_ANTI) invalid("unknown join kind " + std::to_string(kind) + " (a chq_join_kind is expected)");
    require_keys(n_keys, keys, "join");
    require_out_device(out_device);
    std::vector<JoinKeyArg> args((size_t)n_keys);
    for (int k = 0; k < n_keys; ++k) {
      require(keys[k].left, "left join key"); require(keys[k].right, "right join key");
      args[(size_t)k].left = &keys[k].left->e;
      args[(size_t)k].right = &keys[k].right->e;
    }
    using Sides = std::pair<std::vector<Batch>, std::vector<Batch>>;
    phased("chq_join_records_kind", "join",
           [&] {
             require_each(n_left, left, "left record"); require_each(n_right, right, "right record");   // (both sides before either is imported)
             std::vector<Batch> in_l = import_records(n_left, left, left_schema, "left record");
             return Sides(std::move(in_l), import_records(n_right, right, right_schema, "right record"));
           },
           [&](Sides& in) { return join_records(ctx->c, in.first, left_aliases, in.second, right_aliases, args, kind); },
           [&](Batch& res) { finish(ctx->c, std::move(res), out_device, out, out_schema); });
  });
}

// ---- hash partitioning (partition.cpp) -------------------------------------------------------------------------------------
chq_status chq_partition_records(chq_ctx* ctx, int n_records, const ArrowDeviceArray* const* recs, const ArrowSchema* schema,
                                 const chq_table_aliases* table_aliases, const chq_expr* const* keys, int n_keys, int n_partitions,
                                 int out_device, ArrowDeviceArray* outs, ArrowSchema* out_schemas) {
  const bool p_ok = n_partitions >= 1 && n_partitions <= kPartMaxPartitions;   // (else the caller's arrays have no known length)
  return records_entry(ctx, p_ok ? n_partitions : 0, outs, out_schemas, [&] {
    require_records(n_records, recs);
    require_keys(n_keys, keys, "partition");
    if (!p_ok) invalid("n_partitions must be in [1, " + std::to_string(kPartMaxPartitions) + "] (" + std::to_string(n_partitions) + " given)");
    require(outs, "output arrays"); require(out_schemas, "output schemas");
    require_out_device(out_device);
    const std::vector<const Expr*> key_args = expr_args(keys, n_keys, "partition key");
    phased("chq_partition_records", "partition", [&] { return import_records(n_records, recs, schema); },
           [&](std::vector<Batch>& in) { return partition_records(ctx->c, in, table_aliases, key_args, n_partitions); },
           [&](JoinedGroup& res) {
             if (res.ends.size() != (size_t)n_partitions)
               throw ChqError{CHQ_ERR_DEVICE, "internal error: " + std::to_string(res.ends.size()) + " of " + std::to_string(n_partitions) + " partitions"};
             if (out_device == ARROW_DEVICE_CPU) res.joined = to_host(ctx->c, res.joined);
             export_group(std::move(res), out_device, outs, out_schemas);   // every output or none
           });
  });
}

chq_status chq_project_record(chq_ctx* ctx, const chq_select_item* fields, int n_fields, const ArrowDeviceArray* rec,
                              const ArrowSchema* schema, const chq_table_aliases* table_aliases, int out_device,
                              ArrowDeviceArray* out, ArrowSchema* out_schema) {
  return record_entry(ctx, out, out_schema, [&] {
    require_out(out, out_schema);
    const std::vector<chq_select_item> items = select_items(fields, n_fields);
    Batch in = import_batch(rec, schema);
    if (out_device == ARROW_DEVICE_CPU && !in.on_device) {   // the materialize task's calling pattern: host in, host out
      Batch res_host;
      if (project_record_host(ctx->c, items, in, table_aliases, &res_host)) {
        export_batch(std::move(res_host), ARROW_DEVICE_CPU, out, out_schema);
        return;
      }
    }
    DeviceBatch d = device_batch(ctx, in, table_aliases);
    Batch res = project_record(ctx->c, items, d.dev, d.pcols);
    finish(ctx->c, std::move(res), out_device, out, out_schema);
  });
}

chq_status chq_compute_value(chq_ctx* ctx, const ArrowDeviceArray* rec, const ArrowSchema* schema,
                             const chq_table_aliases* table_aliases, const chq_expr* expr, int out_device,
                             ArrowDeviceArray* out, ArrowSchema* out_schema, int* out_is_scalar) {
  return record_entry(ctx, out, out_schema, [&] {
    require(expr, "expression"); require_out(out, out_schema);
    DeviceBatch d = device_batch(ctx, rec, schema, table_aliases);
    bool sc = false;
    Column col = compute_value(ctx->c, d.dev, d.pcols, expr->e, &sc);
    if (out_is_scalar) *out_is_scalar = sc ? 1 : 0;
    // reuse the batch path for the host copy
    Batch one; one.nrows = col.length; one.on_device = true; one.device_id = ctx->c.device;
    one.cols.push_back(std::move(col));
    require_out_device(out_device);
    if (out_device == ARROW_DEVICE_CPU) { Batch h = to_host(ctx->c, one); export_single_column(std::move(h.cols[0]), false, -1, out, out_schema); }
    else export_single_column(std::move(one.cols[0]), true, ctx->c.device, out, out_schema);
  });
}

chq_status chq_filter_project_record(chq_ctx* ctx, const chq_expr* predicate, const chq_select_item* fields, int n_fields,
                                     const ArrowDeviceArray* rec, const ArrowSchema* schema,
                                     const chq_table_aliases* table_aliases, int out_device, ArrowDeviceArray* out,
                                     ArrowSchema* out_schema) {
  return record_entry(ctx, out, out_schema, [&] {
    require(predicate, "predicate"); require_out(out, out_schema);
    const std::vector<chq_select_item> items = select_items(fields, n_fields);
    DeviceBatch d = device_batch(ctx, rec, schema, table_aliases);
    Batch fused;
    if (filter_project_fused(ctx->c, d.dev, d.pcols, predicate->e, items, &fused)) {
      finish(ctx->c, std::move(fused), out_device, out, out_schema);
      return;
    }
    Batch filtered = filter_record(ctx->c, d.dev, d.pcols, predicate->e);   // stays in HBM
    chq_call_stats fs = ctx->c.stats;
    auto pcols2 = plan_columns(filtered, table_aliases);
    Batch res = project_record(ctx->c, items, filtered, pcols2);
    fs.launches += ctx->c.stats.launches;
    ctx->c.stats = fs;
    finish(ctx->c, std::move(res), out_device, out, out_schema);
  });
}

chq_status chq_record_to_device(chq_ctx* ctx, const ArrowDeviceArray* rec, const ArrowSchema* schema, ArrowDeviceArray* out,
                                ArrowSchema* out_schema) {
  return record_entry(ctx, out, out_schema, [&] {
    require_out(out, out_schema);
    Batch in = import_batch(rec, schema, true);   // (staging copies bytes: every fixed width)
    if (in.on_device) invalid("record is already device resident");
    Batch dev = to_device(ctx->c, in);
    check_hip(hipStreamSynchronize(ctx->c.stream), "hipStreamSynchronize");
    export_batch(std::move(dev), ARROW_DEVICE_ROCM, out, out_schema);
  });
}

chq_status chq_record_copy_to_peer(chq_ctx* src_ctx, chq_ctx* dst_ctx, const ArrowDeviceArray* rec, const ArrowSchema* schema,
                                   ArrowDeviceArray* out, ArrowSchema* out_schema) {
  if (!src_ctx) return CHQ_ERR_INVALID_HANDLE;
  return host_entry(dst_ctx, [&] { mark_released(out, out_schema); }, [&] {   // (copy_to_peer makes the destination's GPU current)
    require_out(out, out_schema);
    Batch in = import_batch(rec, schema, true);   // waits on rec->sync_event when the producer left one
    hipEvent_t ev = nullptr;
    Batch moved = copy_to_peer(src_ctx->c, dst_ctx->c, in, &ev);
    export_batch(std::move(moved), ARROW_DEVICE_ROCM, out, out_schema, ev);
  });
}

namespace {
struct IpcHolder { IpcMessage msg; };
void release_ipc(chq_ipc_message* m) {
  if (!m || !m->release) return;
  delete (IpcHolder*)m->private_data;
  memset(m, 0, sizeof(*m));
}
}  // namespace

chq_status chq_record_to_ipc(chq_ctx* ctx, const ArrowDeviceArray* rec, const ArrowSchema* schema, int body_device,
                             chq_ipc_message* out) {
  return entry(ctx, [&] { if (out) memset(out, 0, sizeof(*out)); }, [&] {
    require(out, "output message");
    if (body_device != ARROW_DEVICE_ROCM && body_device != ARROW_DEVICE_CPU) invalid("body_device must be ARROW_DEVICE_CPU or ARROW_DEVICE_ROCM");
    Batch in = import_batch(rec, schema, true);
    Batch dev = to_device(ctx->c, in);   // (a host batch is staged: the body is assembled by the device either way)
    // an unknown null count (-1, a view) stays unknown: the encoder counts it; to_device's "may have nulls" 1 would be written
    for (size_t i = 0; i < dev.cols.size(); ++i) if (in.on_device && in.cols[i].validity && in.cols[i].null_count < 0) dev.cols[i].null_count = -1;
    std::unique_ptr<IpcHolder> h(new IpcHolder());
    h->msg = record_to_ipc(ctx->c, dev, body_device == ARROW_DEVICE_ROCM);
    out->header = h->msg.header.data(); out->header_len = (int64_t)h->msg.header.size();
    out->body = h->msg.body->ptr; out->body_len = h->msg.body_len;
    out->body_device_type = h->msg.body_on_device ? ARROW_DEVICE_ROCM : ARROW_DEVICE_CPU;
    out->body_device_id = h->msg.body_on_device ? ctx->c.device : -1;
    const uint8_t eos[8] = {0xff, 0xff, 0xff, 0xff, 0, 0, 0, 0};
    memcpy(out->end_of_stream, eos, 8);
    out->release = release_ipc; out->private_data = h.release();
  });
}

chq_status chq_record_from_ipc(chq_ctx* ctx, const uint8_t* stream, int64_t stream_len, const void* body, int64_t body_len,
                               int body_device_type, int out_device, ArrowDeviceArray* out, ArrowSchema* out_schema) {
  return record_entry(ctx, out, out_schema, [&] {
    require_out(out, out_schema); require(stream, "stream");
    require_out_device(out_device);
    if (body && body_device_type != ARROW_DEVICE_ROCM && body_device_type != ARROW_DEVICE_CPU)
      invalid("body_device_type must be ARROW_DEVICE_CPU or ARROW_DEVICE_ROCM");
    Batch res = record_from_ipc(ctx->c, stream, stream_len, body, body_len, body_device_type == ARROW_DEVICE_ROCM,
                                out_device == ARROW_DEVICE_ROCM);
    export_batch(std::move(res), out_device, out, out_schema);
  });
}

chq_status chq_ipc_describe(const uint8_t* stream, int64_t stream_len, char* buf, size_t buf_len) {
  return text_result(buf, buf_len, CHQ_ERR_ARROW_INVALID_ARGUMENT, [&] { return describe_ipc(stream, stream_len); });
}

// ---- Parquet scan -------------------------------------------------------------------------------------------------------
chq_status chq_parquet_open(const uint8_t* file, int64_t file_len, chq_parquet** out, char* err, size_t err_len) {
  return open_parquet(out, err, err_len, [&] { return parquet_open(file, file_len); });
}
chq_status chq_parquet_open_reader(int64_t file_len, chq_read_range_fn read, void* user, chq_parquet** out, char* err, size_t err_len) {
  return open_parquet(out, err, err_len, [&] {
    require((const void*)read, "range reader");
    return parquet_open_reader(file_len, read, user);
  });
}
void chq_parquet_close(chq_parquet* pq) { delete pq; }
int32_t chq_parquet_num_columns(const chq_parquet* pq) { return pq ? (int32_t)pq->file.columns.size() : 0; }
const char* chq_parquet_column_name(const chq_parquet* pq, int32_t column) {
  return pq && column >= 0 && column < (int32_t)pq->file.columns.size() ? pq->file.columns[(size_t)column].name.c_str() : nullptr;
}
int32_t chq_parquet_num_row_groups(const chq_parquet* pq) { return pq ? (int32_t)pq->file.row_groups.size() : 0; }
int64_t chq_parquet_row_group_num_rows(const chq_parquet* pq, int32_t row_group) {
  return pq && row_group >= 0 && row_group < (int32_t)pq->file.row_groups.size() ? pq->file.row_groups[row_group].num_rows : -1;
}
chq_status chq_parquet_describe(const chq_parquet* pq, char* buf, size_t buf_len) {
  if (!pq) return CHQ_ERR_INVALID_HANDLE;
  const std::string text = parquet_describe(pq->file);
  copy_text(buf, buf_len, text);
  return text.size() < buf_len ? CHQ_OK : CHQ_ERR_ARROW_INVALID_ARGUMENT;
}
chq_status chq_parquet_read_row_group(chq_ctx* ctx, const chq_parquet* pq, int32_t row_group, int out_device,
                                      ArrowDeviceArray* out, ArrowSchema* out_schema) {
  if (!pq) return CHQ_ERR_INVALID_HANDLE;
  return record_entry(ctx, out, out_schema, [&] {
    require_out(out, out_schema);
    require_out_device(out_device);
    Batch res = parquet_read_row_group(ctx->c, pq->file, row_group);
    if (out_device == ARROW_DEVICE_CPU) res = to_host(ctx->c, res);
    export_batch(std::move(res), out_device, out, out_schema);
  });
}

chq_status chq_parquet_read_row_groups(chq_ctx* ctx, const chq_parquet* pq, int32_t first, int32_t count, int out_device,
                                       ArrowDeviceArray* outs, ArrowSchema* out_schemas) {
  return chq_parquet_read_columns(ctx, pq, first, count, nullptr, -1, out_device, outs, out_schemas);
}

chq_status chq_parquet_read_columns(chq_ctx* ctx, const chq_parquet* pq, int32_t first, int32_t count, const int32_t* columns,
                                    int32_t n_columns, int out_device, ArrowDeviceArray* outs, ArrowSchema* out_schemas) {
  if (!pq) return CHQ_ERR_INVALID_HANDLE;
  return records_entry(ctx, outs && out_schemas ? count : 0, outs, out_schemas, [&] {   // (only a complete pair of arrays is cleared)
    if (count > 0) { require(outs, "output arrays"); require(out_schemas, "output schemas"); }
    require_out_device(out_device);
    if (!columns) n_columns = -1;
    std::vector<Batch> res = parquet_read_row_groups(ctx->c, pq->file, first, count, columns, n_columns);
    const chq_call_stats scan_stats = ctx->c.stats;
    for (size_t i = 0; i < res.size(); ++i) {
      if (out_device == ARROW_DEVICE_CPU) res[i] = to_host(ctx->c, res[i]);
      export_batch(std::move(res[i]), out_device, &outs[i], &out_schemas[i]);
    }
    ctx->c.stats = scan_stats;   // (to_host does not touch them today; the scan's counters are what the call reports)
  });
}

chq_status chq_record_to_parquet(chq_ctx* ctx, const ArrowDeviceArray* rec, const ArrowSchema* schema, chq_parquet_image* out) {
  return image_entry(ctx, out, [&] {
    Batch in = import_batch(rec, schema);
    return record_to_parquet(ctx->c, in);
  });
}

chq_status chq_records_to_parquet(chq_ctx* ctx, int n_records, const ArrowDeviceArray* const* recs, const ArrowSchema* schema,
                                  chq_parquet_image* out) {
  return image_entry(ctx, out, [&] {
    require(recs, "record batches");
    if (n_records < 1) invalid("chq_records_to_parquet needs at least one record batch");
    std::vector<Batch> in((size_t)n_records);
    std::vector<const Batch*> ptrs((size_t)n_records);
    for (int i = 0; i < n_records; ++i) { in[(size_t)i] = import_batch(recs[i], schema); ptrs[(size_t)i] = &in[(size_t)i]; }
    return records_to_parquet(ctx->c, ptrs);
  });
}

chq_status chq_record_to_host(chq_ctx* ctx, const ArrowDeviceArray* rec, const ArrowSchema* schema, ArrowDeviceArray* out,
                              ArrowSchema* out_schema) {
  return record_entry(ctx, out, out_schema, [&] {
    require_out(out, out_schema);
    Batch in = import_batch(rec, schema, true);
    if (!in.on_device) invalid("record is already host resident");
    for (Column& c : in.cols) if (c.validity && c.null_count < 0) c.null_count = 1;
    Batch h = to_host(ctx->c, in);
    // resolve unknown null counts on the host copy
    for (Column& c : h.cols) if (c.validity) c.null_count = count_nulls_host(c.validity, c.offset, c.length);
    export_batch(std::move(h), ARROW_DEVICE_CPU, out, out_schema);
  });
}

chq_status chq_wrap_columns(chq_ctx* ctx, const chq_column_desc* cols, int n_cols, int64_t n_rows, int device_type,
                            ArrowDeviceArray* out, ArrowSchema* out_schema) {
  return host_entry(ctx, [&] { mark_released(out, out_schema); }, [&] {   // (host work only: the caller's current GPU stays)
    require_out(out, out_schema);
    if (n_cols > 0) require(cols, "column descriptors");
    Batch b;
    b.nrows = n_rows; b.on_device = device_type == ARROW_DEVICE_ROCM; b.device_id = ctx->c.device;
    for (int i = 0; i < n_cols; ++i) {
      Column c;
      c.name = cols[i].name ? cols[i].name : ""; c.format = cols[i].format ? cols[i].format : "";
      // validate the format through the importer's table
      ArrowSchema tmp{}; tmp.format = c.format.c_str();
      {
        ArrowSchema parent{}; ArrowSchema* kids[1] = {&tmp}; parent.format = "+s"; parent.n_children = 1; parent.children = kids;
        ArrowArray ka{}; ArrowArray* akids[1] = {&ka}; ArrowDeviceArray da{}; da.array.n_children = 1; da.array.children = akids;
        da.device_type = ARROW_DEVICE_CPU;
        Batch probe = import_batch(&da, &parent);
        c.type = probe.cols[0].type; c.width = probe.cols[0].width;
      }
      if (n_rows > 0 && !cols[i].values) invalid("column '" + c.name + "' has no values buffer");
      if (cols[i].null_count > 0 && !cols[i].validity) invalid("column '" + c.name + "' reports nulls but has no validity bitmap");
      if (n_rows < 0 || cols[i].offset < 0) invalid("negative length or offset");
      c.nullable = cols[i].nullable != 0; c.length = n_rows; c.null_count = cols[i].validity ? cols[i].null_count : 0; c.offset = cols[i].offset;
      c.validity = (const uint8_t*)cols[i].validity; c.values = (const uint8_t*)cols[i].values; c.data = (const uint8_t*)cols[i].data;
      b.cols.push_back(std::move(c));
    }
    export_batch(std::move(b), device_type, out, out_schema);
  });
}

}  // extern "C"
