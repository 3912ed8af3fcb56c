// arrow_io.cpp -- Arrow C Data Interface <-> Batch and <-> the batches of a group, the copies of columns between host and
// device memory, and the plan columns of a batch.
#include "engine_internal.hpp"

#include <atomic>
#include <cstdlib>
#include <cstring>

namespace chq {

namespace {
struct ArrayHolder {
  std::vector<const void*> buffers;
  std::vector<ArrowArray*> child_ptrs;
  std::vector<ArrowArray> children;
  std::vector<BufferPtr> owned;
  hipEvent_t event = nullptr;   // ArrowDeviceArray::sync_event points here when set; destroyed with the array
};
struct SchemaHolder {
  std::string format, name;
  std::vector<ArrowSchema*> child_ptrs;
  std::vector<ArrowSchema> children;
};
void release_array(ArrowArray* a) {
  if (!a || !a->release) return;
  auto* h = (ArrayHolder*)a->private_data;
  if (h) {
    for (auto& c : h->children) if (c.release) c.release(&c);
    if (h->event) { (void)hipEventSynchronize(h->event); (void)hipEventDestroy(h->event); }   // buffers go back to the pool only once the copies behind the event are done
    delete h;
  }
  a->release = nullptr; a->private_data = nullptr;
}
void release_schema(ArrowSchema* s) {
  if (!s || !s->release) return;
  auto* h = (SchemaHolder*)s->private_data;
  if (h) { for (auto& c : h->children) if (c.release) c.release(&c); delete h; }
  s->release = nullptr; s->private_data = nullptr;
}
void fill_column_array(Column&& c, ArrowArray* out) {
  auto* h = new ArrayHolder();
  h->owned = std::move(c.owned);
  const bool keep_validity = c.validity && c.null_count != 0;
  h->buffers.push_back(keep_validity ? c.validity : nullptr);
  h->buffers.push_back(c.values);
  if (c.type == T_UTF8) h->buffers.push_back(c.data);
  memset(out, 0, sizeof(*out));
  out->length = c.length; out->null_count = keep_validity ? c.null_count : 0; out->offset = c.offset;
  out->n_buffers = (int64_t)h->buffers.size(); out->buffers = h->buffers.data();
  out->release = release_array; out->private_data = h;
}
void fill_column_schema(const Column& c, ArrowSchema* out) {
  auto* h = new SchemaHolder();
  h->format = c.format; h->name = c.name;
  memset(out, 0, sizeof(*out));
  out->format = h->format.c_str(); out->name = h->name.c_str();
  out->flags = c.nullable ? ARROW_FLAG_NULLABLE : 0;
  out->release = release_schema; out->private_data = h;
}

// byte range of a bitmap covering bits [offset, offset+len), keeping the sub-byte phase
struct BitRange { int64_t first_byte, nbytes; };
BitRange bit_range(int64_t offset, int64_t len) {
  int64_t fb = offset >> 3, lb = (offset + len + 7) >> 3;
  return {fb, lb - fb};
}
// P2P: `ctx` is the DESTINATION context (buffers on its device, copies on its stream), `peer_device` the GPU `src` lives on
BufferPtr copy_bytes(Context& ctx, const uint8_t* src, int64_t nbytes, Dir dir, size_t pad = 16, int peer_device = -1) {
  BufferPtr out = (dir == Dir::D2H || dir == Dir::H2H) ? make_host_buffer((size_t)nbytes + pad) : make_device_buffer((size_t)nbytes + pad, ctx.device);
  if (dir == Dir::H2H) { if (nbytes > 0) memcpy(out->ptr, src, (size_t)nbytes); return out; }
  if (dir == Dir::P2P) {
    if (nbytes > 0) check_hip(hipMemcpyPeerAsync(out->ptr, ctx.device, src, peer_device, (size_t)nbytes, ctx.stream), "hipMemcpyPeerAsync");
    return out;
  }
  if (nbytes > 0) {
    hipMemcpyKind k = dir == Dir::H2D ? hipMemcpyHostToDevice : (dir == Dir::D2H ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice);
    check_hip(hipMemcpyAsync(out->ptr, src, (size_t)nbytes, k, ctx.stream), "hipMemcpyAsync");
  }
  return out;
}
}  // namespace

// =================================================================================================
// Arrow C Data Interface
// =================================================================================================
const void* Column::values0() const {
  if (type == T_BOOL) return values;
  if (type == T_UTF8) return values ? values + 4 * offset : nullptr;
  return values ? values + (int64_t)width * offset : nullptr;
}

void parse_arrow_format(const char* f, DType* t, int* width, bool copy_only) {
  *width = 0;
  if (f && f[0] && !f[1]) {   // the primitive types are one character: no string object on the per-batch import path
    switch (f[0]) {
      case 'b': *t = T_BOOL; return;
      case 'c': *t = T_I8; *width = 1; return;   case 'C': *t = T_U8; *width = 1; return;
      case 's': *t = T_I16; *width = 2; return;  case 'S': *t = T_U16; *width = 2; return;
      case 'i': *t = T_I32; *width = 4; return;  case 'I': *t = T_U32; *width = 4; return;
      case 'l': *t = T_I64; *width = 8; return;  case 'L': *t = T_U64; *width = 8; return;
      case 'e': *t = T_F16; *width = 2; return;  case 'f': *t = T_F32; *width = 4; return;
      case 'g': *t = T_F64; *width = 8; return;  case 'u': *t = T_UTF8; return;
      default: break;
    }
  }
  const std::string s(f ? f : "");   // multi-character formats: opaque fixed-width types that are only copied
  *t = T_FIXED_OPAQUE;
  if (s == "tdD" || s == "tts" || s == "ttm") { *width = 4; return; }
  if (s == "tdm" || s == "ttu" || s == "ttn" || s.rfind("ts", 0) == 0 || s.rfind("tD", 0) == 0) { *width = 8; return; }
  if (s.rfind("d:", 0) == 0) {   // decimal128 unless a bit width says otherwise
    int commas = (int)std::count(s.begin(), s.end(), ',');
    if (commas == 1) { *width = 16; return; }
    if (commas == 2) { int bw = atoi(s.substr(s.rfind(',') + 1).c_str()); if (bw == 32) { *width = 4; return; } if (bw == 64) { *width = 8; return; } if (bw == 128) { *width = 16; return; } }
  }
  if (s.rfind("w:", 0) == 0) { int w = atoi(s.c_str() + 2); if (w == 1 || w == 2 || w == 4 || w == 8 || w == 16 || (copy_only && w > 0)) { *width = w; return; } }
  throw ChqError{CHQ_ERR_NOT_SUPPORTED, "Arrow type with format '" + s + "' is outside this build's scope"};
}

Batch import_batch(const ArrowDeviceArray* rec, const ArrowSchema* schema, bool copy_only) {
  if (!rec || !schema || !schema->format) throw ChqError{CHQ_ERR_INVALID_HANDLE, "null record batch"};
  if (strcmp(schema->format, "+s") != 0) throw ChqError{CHQ_ERR_ARROW_INVALID_ARGUMENT, "record batch must be a struct array"};
  const ArrowArray& a = rec->array;
  if (a.offset != 0) throw ChqError{CHQ_ERR_NOT_SUPPORTED, "sliced struct arrays are not supported; slice the children"};
  if (a.n_children != schema->n_children) throw ChqError{CHQ_ERR_ARROW_INVALID_ARGUMENT, "schema / array children mismatch"};
  Batch b;
  b.nrows = a.length;
  b.device_id = (int)rec->device_id;
  switch (rec->device_type) {
    case ARROW_DEVICE_CPU: case ARROW_DEVICE_ROCM_HOST: case ARROW_DEVICE_CUDA_HOST: b.on_device = false; break;
    case ARROW_DEVICE_ROCM: b.on_device = true; break;
    default: throw ChqError{CHQ_ERR_NOT_SUPPORTED, "unsupported Arrow device type"};
  }
  if (b.on_device && rec->sync_event) check_hip(hipEventSynchronize(*(hipEvent_t*)rec->sync_event), "hipEventSynchronize(sync_event)");
  b.cols.reserve((size_t)a.n_children);
  for (int64_t i = 0; i < a.n_children; ++i) {
    const ArrowArray* ca = a.children[i];
    const ArrowSchema* cs = schema->children[i];
    if (!ca || !cs) throw ChqError{CHQ_ERR_ARROW_INVALID_ARGUMENT, "missing child array or schema"};
    Column c;
    c.name = cs->name ? cs->name : "";
    c.format = cs->format ? cs->format : "";
    parse_arrow_format(cs->format, &c.type, &c.width, copy_only);
    c.nullable = (cs->flags & ARROW_FLAG_NULLABLE) != 0;
    if (ca->length < b.nrows) throw ChqError{CHQ_ERR_ARROW_INVALID_ARGUMENT, "column shorter than the record batch"};
    if (ca->offset < 0 || b.nrows < 0) throw ChqError{CHQ_ERR_ARROW_INVALID_ARGUMENT, "negative length or offset"};
    // a kernel must never be handed a null data pointer: refuse malformed arrays here, on the host
    if (b.nrows > 0 && (ca->n_buffers < 2 || !ca->buffers || !ca->buffers[1]))
      throw ChqError{CHQ_ERR_ARROW_INVALID_ARGUMENT, std::string("column '") + (cs->name ? cs->name : "") + "' has no values buffer"};
    if (ca->null_count > 0 && (ca->n_buffers < 1 || !ca->buffers[0]))
      throw ChqError{CHQ_ERR_ARROW_INVALID_ARGUMENT, std::string("column '") + (cs->name ? cs->name : "") + "' reports nulls but has no validity bitmap"};
    c.length = b.nrows;
    c.offset = ca->offset;
    c.validity = ca->n_buffers > 0 ? (const uint8_t*)ca->buffers[0] : nullptr;
    c.values = ca->n_buffers > 1 ? (const uint8_t*)ca->buffers[1] : nullptr;
    c.data = ca->n_buffers > 2 ? (const uint8_t*)ca->buffers[2] : nullptr;
    c.null_count = ca->null_count;   // -1 = unknown, resolved when staged
    if (!c.validity) c.null_count = 0;
    if (c.type == T_UTF8 && b.nrows > 0 && !c.data) {
      // legal only when every string is empty; host batches can be checked, device batches are taken at their word
      if (!b.on_device) {
        const int32_t* offs = (const int32_t*)c.values + c.offset;
        if (offs[b.nrows] != offs[0]) throw ChqError{CHQ_ERR_ARROW_INVALID_ARGUMENT, "Utf8 column '" + c.name + "' has offsets but no data buffer"};
      }
    }
    b.cols.push_back(std::move(c));
  }
  return b;
}

void export_batch(Batch&& b, int device_type, ArrowDeviceArray* out, ArrowSchema* out_schema, hipEvent_t sync_event) {
  auto* ah = new ArrayHolder();
  ah->event = sync_event;
  auto* sh = new SchemaHolder();
  const size_t n = b.cols.size();
  ah->children.resize(n); sh->children.resize(n);
  for (size_t i = 0; i < n; ++i) {
    fill_column_schema(b.cols[i], &sh->children[i]);
    fill_column_array(std::move(b.cols[i]), &ah->children[i]);
  }
  for (size_t i = 0; i < n; ++i) { ah->child_ptrs.push_back(&ah->children[i]); sh->child_ptrs.push_back(&sh->children[i]); }
  ah->buffers.push_back(nullptr);
  memset(out, 0, sizeof(*out));
  out->array.length = b.nrows; out->array.null_count = 0; out->array.offset = 0;
  out->array.n_buffers = 1; out->array.buffers = ah->buffers.data();
  out->array.n_children = (int64_t)n; out->array.children = ah->child_ptrs.data();
  out->array.release = release_array; out->array.private_data = ah;
  out->device_id = device_type == ARROW_DEVICE_ROCM ? b.device_id : -1;
  out->device_type = device_type; out->sync_event = ah->event ? (void*)&ah->event : nullptr;
  sh->format = "+s"; sh->name = "";
  memset(out_schema, 0, sizeof(*out_schema));
  out_schema->format = sh->format.c_str(); out_schema->name = sh->name.c_str();
  out_schema->n_children = (int64_t)n; out_schema->children = sh->child_ptrs.data();
  out_schema->release = release_schema; out_schema->private_data = sh;
}

void export_single_column(Column&& c, bool on_device, int device_id, ArrowDeviceArray* out, ArrowSchema* out_schema) {
  fill_column_schema(c, out_schema);
  memset(out, 0, sizeof(*out));
  fill_column_array(std::move(c), &out->array);
  out->device_id = on_device ? device_id : -1;
  out->device_type = on_device ? ARROW_DEVICE_ROCM : ARROW_DEVICE_CPU;
}

void mark_released(ArrowDeviceArray* out, ArrowSchema* out_schema) {
  if (out) { memset(out, 0, sizeof(*out)); }
  if (out_schema) { memset(out_schema, 0, sizeof(*out_schema)); }
}

// ---- the outputs of a joined group call, exported from ONE block --------------------------------------------------------
// Every output batch of such a call is a slice of the same joined buffers (engine.hpp: JoinedGroup).  Exporting them one by
// one (export_batch) costs ~20 allocations per batch and, worse, an atomic reference-count increment per column and batch
// on the SAME few shared buffers from sixteen threads -- 7.5 ms for 12 500 batches, far more than the kernel.  Here the
// Arrow structs of all batches live in a handful of arrays inside one reference-counted block that also holds the buffers:
// exporting a batch writes ~0.6 KB of plain structs, releasing one decrements one counter.
namespace {
struct GroupBlock {
  std::atomic<int64_t> live{0};          // exported structs whose release has not run: (1 + C) arrays + (1 + C) schemas per batch
  std::vector<BufferPtr> buffers;
  std::vector<std::string> names, formats;
  std::string struct_format = "+s", empty;
  // (plain arrays, NOT value-initialised: every element is written by the export loop, which runs on the thread pool -- zero-
  // filling 60 MB of fresh pages on the calling thread first cost 12 ms for 100 000 batches)
  std::unique_ptr<ArrowArray[]> child_arrays;    // [nb * C]
  std::unique_ptr<ArrowArray*[]> child_ptrs;     // [nb * C]
  std::unique_ptr<const void*[]> bufs;           // [nb * C * 3]
  std::unique_ptr<const void*[]> parent_bufs;    // [nb] (the struct array's null validity)
  std::unique_ptr<ArrowSchema[]> child_schemas;  // [nb * C]
  std::unique_ptr<ArrowSchema*[]> schild_ptrs;   // [nb * C]
};
void group_drop(GroupBlock* blk) { if (blk->live.fetch_sub(1, std::memory_order_acq_rel) == 1) delete blk; }
void group_release_child_array(ArrowArray* a) {
  if (!a || !a->release) return;
  auto* blk = (GroupBlock*)a->private_data;
  a->release = nullptr; a->private_data = nullptr;
  group_drop(blk);
}
void group_release_array(ArrowArray* a) {
  if (!a || !a->release) return;
  auto* blk = (GroupBlock*)a->private_data;
  for (int64_t i = 0; i < a->n_children; ++i) if (a->children[i] && a->children[i]->release) a->children[i]->release(a->children[i]);
  a->release = nullptr; a->private_data = nullptr;
  group_drop(blk);
}
void group_release_child_schema(ArrowSchema* s) {
  if (!s || !s->release) return;
  auto* blk = (GroupBlock*)s->private_data;
  s->release = nullptr; s->private_data = nullptr;
  group_drop(blk);
}
void group_release_schema(ArrowSchema* s) {
  if (!s || !s->release) return;
  auto* blk = (GroupBlock*)s->private_data;
  for (int64_t i = 0; i < s->n_children; ++i) if (s->children[i] && s->children[i]->release) s->children[i]->release(s->children[i]);
  s->release = nullptr; s->private_data = nullptr;
  group_drop(blk);
}
}  // namespace

// `outs` / `out_schemas`: one per batch the part covers.  The block goes to the exported structs only once every one of them
// is written; a failure before that frees it and leaves the structs released.
void export_group(JoinedGroup&& g, int device_type, ArrowDeviceArray* outs, ArrowSchema* out_schemas) {
  const size_t nb = g.ends.size(), C = g.joined.cols.size();
  std::unique_ptr<GroupBlock> blk(new GroupBlock());
  try {
    for (Column& c : g.joined.cols) {
      blk->names.push_back(c.name); blk->formats.push_back(c.format);
      for (BufferPtr& b : c.owned) blk->buffers.push_back(std::move(b));
    }
    const size_t cells = std::max<size_t>(1, nb * C);
    blk->child_arrays.reset(new ArrowArray[cells]); blk->child_ptrs.reset(new ArrowArray*[cells]); blk->bufs.reset(new const void*[cells * 3]);
    blk->parent_bufs.reset(new const void*[std::max<size_t>(1, nb)]); blk->child_schemas.reset(new ArrowSchema[cells]); blk->schild_ptrs.reset(new ArrowSchema*[cells]);
    const bool host_out = device_type != ARROW_DEVICE_ROCM;
    GroupBlock* pb = blk.get();
    pool_ranges(nb, 1024, [&](size_t b0, size_t b1) {
      for (size_t b = b0; b < b1; ++b) {
        const int64_t begin = b ? g.ends[b - 1] : 0, rows = g.ends[b] - begin;
        for (size_t i = 0; i < C; ++i) {
          const Column& c = g.joined.cols[i];
          const int64_t at = c.offset + begin;   // the slice's first row in the joined buffers
          ArrowArray& ca = pb->child_arrays[b * C + i];
          const void** cb = &pb->bufs[(b * C + i) * 3];
          memset(&ca, 0, sizeof ca);
          cb[0] = nullptr; cb[2] = nullptr;
          ca.null_count = 0;
          if (c.type == T_UTF8) { cb[1] = c.values; cb[2] = c.data; ca.offset = at; ca.n_buffers = 3; }   // a slice of the joined column
          else if (c.type == T_BOOL || c.validity) { cb[1] = c.values; ca.offset = at; ca.n_buffers = 2; }   // (one Arrow offset serves values and validity)
          else { cb[1] = c.values + at * c.width; ca.offset = 0; ca.n_buffers = 2; }
          if (c.validity) {   // nulls of the slice: unknown on the device (-1), counted for a host result; an all-valid slice drops the bitmap
            cb[0] = c.validity;
            ca.null_count = host_out ? count_nulls_host(c.validity, at, rows) : -1;
            if (ca.null_count == 0) cb[0] = nullptr;
          }
          ca.length = rows; ca.buffers = cb; ca.release = group_release_child_array; ca.private_data = pb;
          pb->child_ptrs[b * C + i] = &ca;
          ArrowSchema& cs = pb->child_schemas[b * C + i];
          memset(&cs, 0, sizeof cs);
          cs.format = pb->formats[i].c_str(); cs.name = pb->names[i].c_str(); cs.flags = c.nullable ? ARROW_FLAG_NULLABLE : 0;
          cs.release = group_release_child_schema; cs.private_data = pb;
          pb->schild_ptrs[b * C + i] = &cs;
        }
        ArrowDeviceArray& o = outs[b];
        memset(&o, 0, sizeof o);
        pb->parent_bufs[b] = nullptr;
        o.array.length = rows; o.array.n_buffers = 1; o.array.buffers = &pb->parent_bufs[b];
        o.array.n_children = (int64_t)C; o.array.children = C ? &pb->child_ptrs[b * C] : nullptr;
        o.array.release = group_release_array; o.array.private_data = pb;
        o.device_id = device_type == ARROW_DEVICE_ROCM ? g.joined.device_id : -1; o.device_type = device_type; o.sync_event = nullptr;
        ArrowSchema& os = out_schemas[b];
        memset(&os, 0, sizeof os);
        os.format = pb->struct_format.c_str(); os.name = pb->empty.c_str();
        os.n_children = (int64_t)C; os.children = C ? &pb->schild_ptrs[b * C] : nullptr;
        os.release = group_release_schema; os.private_data = pb;
      }
    });
  } catch (...) {
    for (size_t b = 0; b < nb; ++b) mark_released(&outs[b], &out_schemas[b]);
    throw;
  }
  blk->live.store((int64_t)(nb * (2 + 2 * C)));
  (void)blk.release();
}

// ---- GroupLite: the per-batch facts of a group (group_plan.hpp) -------------------------------------------------------------
// `set` reads an imported batch, `set_from_arrow` the Arrow structs of a device batch (the checks of import_batch, but no
// Batch object).  Both run per batch on the pool's threads and allocate nothing.  They must agree on: the residency bits,
// GL_SHORT below 2 rows, GL_SCHEMA_DIFFERS for anything the group paths cannot take (the full import then decides and
// reports), and per column what `put_column` stores.
void GroupLite::set(size_t b, const Batch& r, const Batch& first, int device) {
  rows[b] = r.nrows;
  uint8_t f = 0;
  if (!r.on_device) f |= GL_ON_HOST;
  if (r.on_device && r.device_id == device) f |= GL_ON_DEVICE;
  if (r.nrows < 2) f |= GL_SHORT;
  if (r.cols.size() != ncols) { flags[b] = (uint8_t)(f | GL_SCHEMA_DIFFERS); return; }
  for (size_t i = 0; i < ncols; ++i) {
    const Column& c = r.cols[i];
    const Column& c0 = first.cols[i];
    if (c.type != c0.type || c.width != c0.width || c.format != c0.format) f |= GL_SCHEMA_DIFFERS;
    f |= put_column(b * ncols + i, GroupCol{c.type, c.width}, !r.on_device, c.validity, c.null_count, c.length, c.values, c.data, c.offset);
  }
  flags[b] = f;
}

void GroupLite::set_from_arrow(size_t b, const ArrowDeviceArray* rec, const ArrowSchema* schema, const Batch& first, int device) {
  const ArrowArray& a = rec->array;
  if (a.offset != 0 || a.n_children != schema->n_children || (size_t)a.n_children != ncols || rec->device_type != ARROW_DEVICE_ROCM || rec->sync_event) {
    flags[b] = GL_SCHEMA_DIFFERS;   // (anything unusual: the full import decides -- and reports)
    return;
  }
  rows[b] = a.length;
  uint8_t f = 0;
  if ((int)rec->device_id == device) f |= GL_ON_DEVICE;
  if (a.length < 2) f |= GL_SHORT;
  for (size_t i = 0; i < ncols; ++i) {
    const ArrowArray* ca = a.children[i];
    if (!ca || ca->length < a.length || ca->offset < 0 || ca->n_buffers < 2 || !ca->buffers || !ca->buffers[1] ||
        (ca->null_count > 0 && !ca->buffers[0])) { f |= GL_SCHEMA_DIFFERS; continue; }
    const Column& c0 = first.cols[i];
    const uint8_t* bytes = c0.type == T_UTF8 && ca->n_buffers > 2 ? (const uint8_t*)ca->buffers[2] : nullptr;
    f |= put_column(b * ncols + i, GroupCol{c0.type, c0.width}, false, (const uint8_t*)ca->buffers[0], ca->null_count, a.length, (const uint8_t*)ca->buffers[1], bytes, ca->offset);
  }
  flags[b] = f;
}

// Import of a group.  Batch 0 is imported in full.  A DEVICE-resident group then only gathers its GroupLite -- the checks of
// import_batch on every record, but no Batch objects: the one-launch path works from the flat arrays, and building and
// freeing 12 500 Batch objects cost ~0.6 ms of a 2.5 ms call; `gi.materialise` imports them when another path needs them.
// Host groups are imported in full, and described by their GroupLite like any other.
void import_group(int n_records, const ArrowDeviceArray* const* recs, const ArrowSchema* schema, int device, GroupInput& gi) {
  std::vector<Batch>& in = gi.batches;
  GroupLite& lite = gi.lite;
  in.resize(1);
  in[0] = import_batch(recs[0], schema);
  lite.resize((size_t)n_records, in[0].cols.size());
  lite.set(0, in[0], in[0], device);
  auto import_rest = [n_records, recs, schema, &in]() {
    if ((int)in.size() == n_records) return;
    in.resize((size_t)n_records);
    if (n_records > 1) for_each_parallel(n_records - 1, [&](int k) { in[(size_t)k + 1] = import_batch(recs[(size_t)k + 1], schema); });
  };
  if (in[0].on_device && n_records > 1) {
    const Batch& first = in[0];
    for_each_parallel(n_records - 1, [&](int k) { lite.set_from_arrow((size_t)k + 1, recs[(size_t)k + 1], schema, first, device); });
    gi.materialise = import_rest;
    return;
  }
  import_rest();
  const Batch& first = in[0];
  if (n_records > 1) for_each_parallel(n_records - 1, [&](int k) { lite.set((size_t)k + 1, in[(size_t)k + 1], first, device); });
}

// =================================================================================================
// host <-> device staging
// =================================================================================================
// Copy one column across (or within) memory spaces; the copy keeps `offset & 7` so that validity,
// boolean values and value buffers share one Arrow offset.
Column copy_column(Context& ctx, const Column& c, Dir dir, int peer_device) {
  auto copy_bytes = [peer_device](Context& cx, const uint8_t* src, int64_t nbytes, Dir d, size_t pad = 16) {
    return chq::copy_bytes(cx, src, nbytes, d, pad, peer_device);
  };
  Column o;
  o.name = c.name; o.format = c.format; o.type = c.type; o.width = c.width; o.nullable = c.nullable;
  o.length = c.length; o.null_count = c.null_count;
  const int64_t phase = c.offset & 7, base = c.offset - phase, n = c.length;
  o.offset = phase;
  if (c.validity && c.null_count != 0) {
    BitRange r = bit_range(c.offset, n);
    auto vb = copy_bytes(ctx, c.validity + r.first_byte, r.nbytes, dir);
    o.validity = (const uint8_t*)vb->ptr; o.owned.push_back(vb);
  }
  if (c.type == T_BOOL) {
    BitRange r = bit_range(c.offset, n);
    auto b = copy_bytes(ctx, c.values + r.first_byte, r.nbytes, dir);
    o.values = (const uint8_t*)b->ptr; o.owned.push_back(b);
  } else if (c.type == T_UTF8) {
    // offsets [base, offset+n]; data bytes [off[offset], off[offset+n]) -- need the two end offsets on the host
    int32_t ends[2] = {0, 0};
    if (c.values) {
      if (dir == Dir::H2D || dir == Dir::H2H) { const int32_t* offs = (const int32_t*)c.values; ends[0] = offs[c.offset]; ends[1] = offs[c.offset + n]; }
      else {   // (unified addressing: the copy finds the source GPU from the pointer, also for a peer's memory)
        check_hip(hipMemcpyAsync(&ends[0], c.values + 4 * c.offset, 4, hipMemcpyDeviceToHost, ctx.stream), "read offsets");
        check_hip(hipMemcpyAsync(&ends[1], c.values + 4 * (c.offset + n), 4, hipMemcpyDeviceToHost, ctx.stream), "read offsets");
        check_hip(hipStreamSynchronize(ctx.stream), "sync");
      }
    }
    auto ob = c.values ? copy_bytes(ctx, c.values + 4 * base, 4 * (n + phase + 1), dir) : copy_bytes(ctx, nullptr, 0, dir);
    if (!c.values) {   // empty array without an offsets buffer: synthesise [0]
      int32_t zero[9] = {0};
      if (dir == Dir::D2H || dir == Dir::H2H) memcpy(ob->ptr, zero, sizeof zero); else check_hip(hipMemcpyAsync(ob->ptr, zero, 16, hipMemcpyHostToDevice, ctx.stream), "memcpy");
    }
    o.values = (const uint8_t*)ob->ptr; o.owned.push_back(ob);
    const int64_t nb = (int64_t)ends[1] - ends[0];
    auto db = copy_bytes(ctx, c.data ? c.data + ends[0] : nullptr, c.data ? nb : 0, dir);
    o.data = (const uint8_t*)db->ptr - ends[0];   // offsets stay absolute
    o.data_bytes = nb;
    o.owned.push_back(db);
  } else {
    auto b = copy_bytes(ctx, c.values ? c.values + (int64_t)c.width * base : nullptr, c.values ? (int64_t)c.width * (n + phase) : 0, dir);
    o.values = (const uint8_t*)b->ptr; o.owned.push_back(b);
  }
  return o;
}

Batch to_device(Context& ctx, const Batch& b) {
  Batch o;
  o.nrows = b.nrows; o.on_device = true; o.device_id = ctx.device;
  for (const Column& c : b.cols) {
    Column cc = c;
    if (!b.on_device) {
      if (cc.validity && cc.null_count < 0) cc.null_count = count_nulls_host(cc.validity, cc.offset, cc.length);
      o.cols.push_back(copy_column(ctx, cc, Dir::H2D));
    } else {
      if (cc.validity && cc.null_count < 0) cc.null_count = 1;   // unknown: assume nulls may be present
      o.cols.push_back(cc);   // view, nothing owned
    }
  }
  return o;
}

Batch copy_to_peer(Context& src, Context& dst, const Batch& b, hipEvent_t* event_out) {
  if (!b.on_device) throw ChqError{CHQ_ERR_ARROW_INVALID_ARGUMENT, "chq_record_copy_to_peer moves device-resident batches; stage host batches with chq_record_to_device on the destination context"};
  check_hip(hipSetDevice(dst.device), "hipSetDevice");
  if (src.device != dst.device) {   // direct xGMI path between the pair (the copy is staged through the host without it)
    int can = 0;
    if (hipDeviceCanAccessPeer(&can, dst.device, src.device) == hipSuccess && can) {
      const hipError_t e = hipDeviceEnablePeerAccess(src.device, 0);
      if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) check_hip(e, "hipDeviceEnablePeerAccess");
      (void)hipGetLastError();
    }
  }
  Batch o;
  o.nrows = b.nrows; o.on_device = true; o.device_id = dst.device;
  for (const Column& c : b.cols) {
    Column cc = c;
    if (cc.validity && cc.null_count < 0) cc.null_count = 1;   // unknown: keep the bitmap
    o.cols.push_back(copy_column(dst, cc, Dir::P2P, src.device));
  }
  hipEvent_t ev = nullptr;
  check_hip(hipEventCreateWithFlags(&ev, hipEventDisableTiming), "hipEventCreate");
  const hipError_t e = hipEventRecord(ev, dst.stream);
  if (e != hipSuccess) { (void)hipEventDestroy(ev); check_hip(e, "hipEventRecord"); }
  *event_out = ev;
  return o;
}

Batch to_host(Context& ctx, const Batch& b) {
  Batch o;
  o.nrows = b.nrows; o.on_device = false; o.device_id = -1;
  for (const Column& c : b.cols) o.cols.push_back(b.on_device ? copy_column(ctx, c, Dir::D2H) : c);
  check_hip(hipStreamSynchronize(ctx.stream), "hipStreamSynchronize");
  return o;
}

std::vector<PlanColumn> plan_columns(const Batch& b, const chq_table_aliases* aliases) {
  std::vector<PlanColumn> out;
  for (size_t i = 0; i < b.cols.size(); ++i) {
    PlanColumn p;
    p.name = b.cols[i].name; p.type = b.cols[i].type; p.format = b.cols[i].format; p.width = b.cols[i].width;
    p.has_nulls = b.cols[i].validity && b.cols[i].null_count != 0;
    // without an explicit table_aliases argument every column has an (empty) alias list
    p.alias_entry_present = aliases ? (int)i < aliases->n_columns : true;
    if (aliases && (int)i < aliases->n_columns)
      for (int k = 0; k < aliases->columns[i].n; ++k) p.aliases.push_back(aliases->columns[i].aliases[k]);
    out.push_back(std::move(p));
  }
  return out;
}

}  // namespace chq
