// filter.cpp -- the single-batch filter: encoding and launching a lowered program, typing, the uniform-length Utf8 rewrite,
// filter_record stage by stage and the two host fast paths.  (Expressions that do not fit one program: materialize.cpp.)
// Reference map: filter_record = RU/filter_record.rs:21-39 (RU = src/handlers/operator_handler/operators/record_utils of the
// reference).
#include "engine_internal.hpp"

#include <condition_variable>
#include <cstring>
#include <deque>
#include <exception>
#include <mutex>
#include <thread>

namespace chq {

namespace {

constexpr int kStashSlots[3] = {STASH_SLOTS_K0, STASH_SLOTS_K1, STASH_SLOTS_K2};

// FAST_UOPS (device_program.h): pre-decode a program whose every instruction works on non-null Int32 / UInt32 / Float32
// columns, 32-bit literals and boolean temporaries into (operand kind, loop body) pairs.  Returns false -- the generic
// interpreter runs -- as soon as one instruction falls outside that set.
bool encode_fast_uops(ProgramBlock& pb, const Lowered& lw, const Batch& rec) {
  if (lw.wide || lw.num_temps > 0 || !lw.strs.empty() || lw.prog.empty()) return false;
  auto is32 = [](int t) { return t == T_I32 || t == T_U32 || t == T_F32; };
  bool nullable_ref = false;
  for (int ci : lw.refs) {
    const Column& c = rec.cols[ci];
    if (!is32(c.type)) return false;
    nullable_ref |= c.validity && c.null_count != 0;
  }
  if (nullable_ref) {
    // columns WITH nulls: only `column <cmp> literal` (LOAD col; CMP const) -- the predicate of most sample queries, and Parquet
    // `optional` columns with real nulls are the normal case off read_files -- keeps the fast evaluators (they AND the column's
    // validity into the result; their boolean temporaries carry none, so anything longer takes the generic interpreter)
    const bool cmp_const = lw.prog.size() == 2 && lw.refs.size() == 1 && lw.prog[0].op == OP_LOAD && lw.prog[0].src_kind == SRC_COL &&
                           lw.prog[0].src_type == lw.prog[0].type && lw.prog[1].op >= OP_EQ && lw.prog[1].op <= OP_GE &&
                           lw.prog[1].src_kind == SRC_CONST && lw.prog[1].type == lw.prog[0].type;
    if (!cmp_const) return false;
  }
  for (size_t i = 0; i < lw.prog.size(); ++i) {
    const Instr& in = pb.prog[i];   // (never modified: incomplete waves run the same program through the generic interpreter)
    const bool rev = in.flags & IF_REV;
    uint8_t opd = FO_NONE, fop = FU_NOPS;
    bool negate = false;
    // ---- operand ----
    if (in.src_kind == SRC_COL) {
      if (!is32(in.src_type)) return false;
      if (in.src_type == in.type) opd = FO_COL;
      else if (in.type == T_F32 && in.src_type == T_I32) opd = FO_COL_I2F;
      else if (in.type == T_F32 && in.src_type == T_U32) opd = FO_COL_U2F;
      else return false;
    } else if (in.src_kind == SRC_CONST) {
      if (!is32(in.type) && !(in.op == OP_LOAD && in.type == T_BOOL)) return false;
      if (in.type == T_BOOL) return false;   // boolean literals take the generic path (length rules make them rare)
      opd = FO_CONST;
    } else if (in.src_kind == SRC_TEMP) {
      if (in.src_type != T_BOOL || in.src_idx >= MAX_BOOL_TEMPS) return false;
      opd = FO_BTEMP;
    }
    // ---- operation ----
    const uint32_t c = (uint32_t)in.imm;
    const bool pow2 = opd == FO_CONST && !rev && c != 0 && c <= 0x40000000u && (c & (c - 1)) == 0;
    switch (in.op) {
      case OP_LOAD:
        if (opd == FO_NONE) return false;
        if (opd == FO_BTEMP && in.type != T_BOOL) return false;
        fop = FU_LD;
        break;
      case OP_ADD: case OP_MUL: case OP_SUB: case OP_DIV: case OP_REM: {
        if (opd == FO_BTEMP || opd == FO_NONE) return false;
        const bool add = in.op == OP_ADD, mul = in.op == OP_MUL, sub = in.op == OP_SUB, div = in.op == OP_DIV;
        if (in.type == T_F32) {
          if (add) fop = FU_ADD_F; else if (mul) fop = FU_MUL_F; else if (sub) fop = rev ? FU_RSUB_F : FU_SUB_F;
          else if (div) fop = rev ? FU_RDIV_F : FU_DIV_F; else return false;   // fmod: generic path
        } else if (in.type == T_I32 || in.type == T_U32) {
          const bool s = in.type == T_I32;
          if (add) fop = s ? FU_ADD_I : FU_ADD_U; else if (mul) fop = s ? FU_MUL_I : FU_MUL_U;
          else if (sub) fop = rev ? (s ? FU_RSUB_I : FU_RSUB_U) : (s ? FU_SUB_I : FU_SUB_U);
          else if (pow2) fop = div ? (s ? FU_DIVP2_I : FU_DIVP2_U) : (s ? FU_REMP2_I : FU_REMP2_U);
          else return false;   // general integer division: generic path
        } else return false;
      } break;
      case OP_EQ: case OP_NE: case OP_LT: case OP_LE: case OP_GT: case OP_GE: {
        if (opd == FO_BTEMP || opd == FO_NONE || !is32(in.type)) return false;
        // primitives on (x = accumulator, y = operand): EQ, LT (x < y), GT (x > y); `rev` = operand (op) accumulator
        bool lt = false;   // else gt
        switch (in.op) {
          case OP_EQ: fop = FU_EQ; break;
          case OP_NE: fop = FU_EQ; negate = true; break;
          case OP_LT: lt = !rev; fop = 1; break;
          case OP_GT: lt = rev; fop = 1; break;
          case OP_LE: lt = rev; negate = true; fop = 1; break;    // x <= y == !(x > y)
          default: lt = !rev; negate = true; fop = 1; break;      // x >= y == !(x < y)
        }
        if (fop == 1) {
          if (in.type == T_I32) fop = lt ? FU_LT_I : FU_GT_I;
          else if (in.type == T_U32) fop = lt ? FU_LT_U : FU_GT_U;
          else if (opd == FO_CONST && (int32_t)c >= 0) fop = lt ? FU_LT_I : FU_GT_I;   // raw bits order like the keys (kernels.hip: run_cmp_const)
          else if (opd == FO_CONST) fop = lt ? FU_LT_FKC : FU_GT_FKC;   // (the device keys the literal once per instruction)
          else fop = lt ? FU_LT_F : FU_GT_F;
        }
      } break;
      case OP_AND: case OP_OR:
        if (opd != FO_BTEMP) return false;
        fop = in.op == OP_AND ? FU_AND : FU_OR;
        break;
      case OP_SPILL:
        if (in.type != T_BOOL || in.src_idx >= MAX_BOOL_TEMPS) return false;
        fop = FU_SPILL; opd = FO_NONE;
        break;
      case OP_CAST:
        if (in.type == T_F32 && in.src_type == T_I32) fop = FU_CVT_I2F;
        else if (in.type == T_F32 && in.src_type == T_U32) fop = FU_CVT_U2F;
        else return false;
        opd = FO_NONE;
        break;
      case OP_STORE: fop = FU_STORE; opd = FO_NONE; break;
      default: return false;
    }
    pb.fast_op[i] = (uint8_t)(fop | (negate ? FU_NEGATE : 0));
    pb.fast_opd[i] = opd;
  }
  return true;
}

// (a Float16 operand reaches the stash widened to f32: not the column's bytes)
bool stashable(const Column& c) { return c.type != T_BOOL && c.type != T_UTF8 && c.type != T_F16 && c.width > 0 && c.width <= 4; }

// ---- filter_record, stage by stage ---------------------------------------------------------------------------------------
constexpr size_t kNullPerRound = 16, kUtf8PerRound = 8;   // follow-up rounds: null counters / Utf8 columns per read-back
// Stage 1, typing and lowering.  `rec`: what the program's column refs index, the batch or (fit_to_device) `work`.
struct FilterProgram { Lowered lw; int64_t mask_len = 0; const Batch* rec = nullptr; Batch work; std::vector<PlanColumn> wcols; TypedExpr fitted; };
void type_filter(Context& ctx, const Batch& rec, const std::vector<PlanColumn>& pcols, const Expr& expr, FilterProgram& fp) {
  const int64_t nrows = rec.nrows;
  TypedExpr te = typed(ctx, rec, pcols, expr);
  if (te.nodes[(size_t)te.root].kind == Node::CONST && te.nodes[(size_t)te.root].cval.null) {
    Scalar& v = te.nodes[(size_t)te.root].cval;   // a NULL mask slot drops its row (prep_null_mask_filter)
    v.null = false; v.bits = 0;
  }
  const Node& root = te.at(te.root);
  if (root.type != T_BOOL) {   // RU/filter_record.rs:27-35
    // the reference has already evaluated the expression at this point: data-dependent errors come first
    if (root.kind != Node::COL && !root.len1 && nrows > 0) { std::vector<const TypedExpr*> v{&te}; (void)evaluate_dense(ctx, rec, pcols, v); }
    throw ChqError{CHQ_ERR_CAST_TO_BOOLEAN_ARRAY_FAILED, std::string("cast to boolean array failed for array type: ") + dtype_name(root.type)};
  }
  // A literal-only predicate is a length-1 mask: arrow filters just the first row (and rejects a mask
  // longer than the columns) -- reproduced, not "fixed" (SURVEY.md section 8 a8).
  fp.mask_len = root.len1 ? 1 : nrows;
  if (fp.mask_len > nrows && !rec.cols.empty())
    throw ChqError{CHQ_ERR_ARROW_INVALID_ARGUMENT, "Filter predicate of length " + std::to_string(fp.mask_len) +
                                                       " is larger than target array of length " + std::to_string(nrows)};
  fp.rec = &rec;
  try {
    lower_expr(te, te.root, pcols, fp.lw);
  } catch (const ChqError& e) {
    if (e.code != CHQ_INTERNAL_PROGRAM_LIMIT) throw;
    fit_to_device(ctx, rec, pcols, te, fp.work, fp.wcols, fp.fitted);   // sub-trees -> temporary columns until the rest fits
    fp.lw = Lowered{};
    lower_expr(fp.fitted, fp.fitted.root, fp.wcols, fp.lw);
    fp.rec = &fp.work;
  }
}

// Stage 2, the uniform-length Utf8 detour.  Utf8 columns whose values all have the same length (keys, hashes, dates as text,
// the reference's own sample strings -- create_sample_data.rs) are fixed-width columns in disguise: value i lies at
// data + offsets[0] + i L.  One cheap pass over the offsets proves it (4 B/row); the column then goes through the fixed-width
// copy of the main kernel (whole 8- or 16-byte values per lane) instead of the per-row string scatter, and its new offsets
// are 0, L, 2 L, ...  Config-5 shape: 0.99 -> 0.6 ms per 125 M-row batch.  Only columns the predicate does not read, without
// nulls.  True: `*res` is the call's result.
bool uniform_detour(Context& ctx, const Batch& rec, const std::vector<PlanColumn>& pcols, const Expr& expr, SplitRequest* split,
                    const FilterProgram& fp, Batch* res) {
  const int64_t nrows = rec.nrows;
  if (fp.rec != &rec || fp.mask_len != nrows || ctx.opt_uniform_utf8_rows <= 0 || nrows < ctx.opt_uniform_utf8_rows || !rec.on_device) return false;
  std::vector<int> cand;
  for (size_t i = 0; i < rec.cols.size(); ++i) {
    const Column& c = rec.cols[i];
    if (c.type != T_UTF8 || !c.values || !c.data || !uniform_utf8_ok(c.validity && c.null_count != 0, nrows, 1)) continue;
    if (std::find(fp.lw.refs.begin(), fp.lw.refs.end(), (int)i) != fp.lw.refs.end()) continue;
    cand.push_back((int)i);
  }
  if (cand.empty()) return false;
  // (with `time_kernels` the check and the offsets kernels are timed too and added to the call's kernel time: the
  // roofline of this path must not be flattered by leaving its extra passes out)
  auto d_chk = make_device_buffer(cand.size() * 16 + 16, ctx.device);
  check_hip(hipMemsetAsync(d_chk->ptr, 0, cand.size() * 16, ctx.stream), "memset");
  kernel_span_begin(ctx);
  for (size_t k = 0; k < cand.size(); ++k) {
    Utf8UniformParams up{(const int32_t*)rec.cols[(size_t)cand[k]].values0(), nrows, (int32_t*)d_chk->ptr + 4 * k};
    check_hip(launch_utf8_uniform(up, ctx.stream), "launch utf8_uniform_kernel");
  }
  kernel_span_end(ctx);
  std::vector<int32_t> h_chk(cand.size() * 4);
  check_hip(hipMemcpyAsync(h_chk.data(), d_chk->ptr, cand.size() * 16, hipMemcpyDeviceToHost, ctx.stream), "read back");
  check_hip(hipStreamSynchronize(ctx.stream), "hipStreamSynchronize");
  const int64_t check_ns = kernel_span_ns(ctx);   // (now: the inner call reuses the events)
  Batch view = rec;
  std::vector<PlanColumn> vcols = pcols;
  std::vector<int> turned;
  for (size_t k = 0; k < cand.size(); ++k) {
    const int32_t differs = h_chk[4 * k], len = h_chk[4 * k + 1], first = h_chk[4 * k + 2];
    if (differs || first < 0 || !uniform_utf8_ok(false, nrows, len)) continue;
    Column& v = view.cols[(size_t)cand[k]];
    v.type = T_FIXED_OPAQUE; v.format = "w:" + std::to_string(len); v.width = len;
    v.values = v.data + first; v.data = nullptr; v.data_bytes = -1; v.offset = 0; v.validity = nullptr; v.null_count = 0;
    PlanColumn& vc = vcols[(size_t)cand[k]];
    vc.type = T_FIXED_OPAQUE; vc.format = v.format; vc.width = len; vc.has_nulls = false;
    turned.push_back(cand[k]);
  }
  if (turned.empty()) return false;
  *res = filter_record(ctx, view, vcols, expr, split);   // (no eligible Utf8 column is left in the view: no further recursion)
  kernel_span_begin(ctx);
  for (int ci : turned) {
    Column& o = res->cols[(size_t)ci];
    o = uniform_to_utf8(ctx, std::move(o), rec.cols[(size_t)ci], res->nrows, true);   // (counts the offsets written)
    ctx.stats.bytes_read_alg += (nrows + 1) * 4;   // the offsets were read by the check
  }
  kernel_span_end(ctx);
  check_hip(hipStreamSynchronize(ctx.stream), "hipStreamSynchronize");
  ctx.stats.kernel_ns += check_ns + kernel_span_ns(ctx);
  ctx.stats.launches += (int64_t)(cand.size() + turned.size());
  return true;
}

// Stage 3: empty in, empty out (schema preserved)
Batch empty_filter_result(Context& ctx, const Batch& rec) {
  Batch out;
  out.on_device = true; out.device_id = ctx.device; out.nrows = 0;
  for (const Column& c : rec.cols) {
    Column o = empty_like(c);
    give_empty_buffers(ctx, o);
    out.cols.push_back(std::move(o));
  }
  check_hip(hipStreamSynchronize(ctx.stream), "sync");
  return out;
}

// Stages 4 to 7 of one call: launch geometry, columns by kind, the fold plan, the selection bitmap and the output
struct FilterCall {
  Context& ctx; const Batch& rec; const FilterProgram& fp; SplitRequest* split;
  int tile_kind;
  int64_t mask_len, tile_rows, ntiles, ngroups, total = 0;
  std::vector<BufferPtr> str_bufs;
  std::vector<int> fixed_cols, bool_cols, utf8_cols, nullable_cols;   // (utf8_cols: those the follow-up rounds filter)
  std::vector<int> fold_cols; std::vector<int64_t> fold_cap; std::vector<bool> fold_data;   // filtered by the main kernel
  std::vector<BufferPtr> fold_status;
  bool need_followup = false;   // (then the main kernel writes the selection bitmap)
  BufferPtr sel_mask, grp_base;
  Batch out;

  FilterCall(Context& c, const Batch& r, const FilterProgram& p, SplitRequest* s)
      : ctx(c), rec(r), fp(p), split(s), tile_kind(pick_tile_kind(c, p.lw, p.mask_len)), mask_len(p.mask_len), tile_rows(kTileRows[tile_kind]),
        ntiles((mask_len + tile_rows - 1) / tile_rows), ngroups((mask_len + 63) / 64) {
    out.on_device = true; out.device_id = ctx.device;
    for (const Column& col : rec.cols) out.cols.push_back(empty_like(col));
    ensure_scratch(ctx, ntiles);
    str_bufs = upload_strings(ctx, fp.lw);
    for (size_t i = 0; i < rec.cols.size(); ++i) {
      const Column& col = rec.cols[i];
      if (col.type == T_BOOL) bool_cols.push_back((int)i);
      else if (col.type == T_UTF8) utf8_cols.push_back((int)i);
      else fixed_cols.push_back((int)i);
      if (col.validity && col.null_count != 0) nullable_cols.push_back((int)i);
    }
  }
  void plan_fold(); void launch_main(); void read_main(); void follow_ups();   // (the stages)
  // first / last input offset of Utf8 columns [u0, u1) into the scratch header: their outputs' byte capacity
  void gather_utf8_ends(size_t u0, size_t u1) {
    if (u1 <= u0) return;
    GatherParams gp{};
    for (size_t k = u0; k < u1; ++k) {
      const int32_t* offs = (const int32_t*)rec.cols[utf8_cols[k]].values0();
      gp.src[2 * (k - u0)] = offs; gp.src[2 * (k - u0) + 1] = offs + mask_len;
    }
    gp.n = (int32_t)(2 * (u1 - u0)); gp.dst = dev_scratch(ctx)->utf8_ends;
    check_hip(launch_gather_i32(gp, ctx.stream), "launch gather_i32_kernel");
  }
};

// Stage 4, the fold plan.  Utf8 columns of short strings are filtered inside the main kernel (device_program.h: Utf8Fold).
// Their output capacity is the input byte span: known when the library built the column itself (staged, joined, decoded),
// one 8-byte read-back otherwise.  Long strings (more than 24 bytes per row on average) get only their new offsets from the
// main kernel; the bytes are moved by utf8_copy_kernel (one wave per 64 rows), launched right behind it.
void FilterCall::plan_fold() {
  if (ctx.opt_fold_utf8 && tile_kind != 2 && !utf8_cols.empty() && mask_len == rec.nrows) {
    const size_t ncand = std::min<size_t>(MAX_FOLD_UTF8, utf8_cols.size());
    std::vector<int64_t> cap(ncand, -1);
    bool unknown = false;
    for (size_t k = 0; k < ncand; ++k) { cap[k] = rec.cols[utf8_cols[k]].data_bytes; unknown |= cap[k] < 0; }
    if (unknown) {
      Scratch* ds = dev_scratch(ctx);
      Scratch* hs = (Scratch*)ctx.pinned.ptr;
      gather_utf8_ends(0, ncand);
      check_hip(hipMemcpyAsync(hs->utf8_ends, ds->utf8_ends, sizeof(hs->utf8_ends), hipMemcpyDeviceToHost, ctx.stream), "read back");
      check_hip(hipStreamSynchronize(ctx.stream), "hipStreamSynchronize");
      for (size_t k = 0; k < ncand; ++k) cap[k] = (int64_t)hs->utf8_ends[2 * k + 1] - hs->utf8_ends[2 * k];
    }
    std::vector<int> rest;
    for (size_t k = 0; k < utf8_cols.size(); ++k) {
      if (k < ncand) { fold_cols.push_back(utf8_cols[k]); fold_cap.push_back(cap[k]); fold_data.push_back(cap[k] <= mask_len * 24); }
      else rest.push_back(utf8_cols[k]);
    }
    utf8_cols.swap(rest);
  }
  const bool fold_long = std::find(fold_data.begin(), fold_data.end(), false) != fold_data.end();
  need_followup = !bool_cols.empty() || !utf8_cols.empty() || !nullable_cols.empty() || (int)fixed_cols.size() > MAX_OUT ||
                    (split && !split->starts.empty()) || fold_long;
  if (need_followup) {
    sel_mask = make_device_buffer((size_t)(ngroups + 2) * 8, ctx.device);
    grp_base = make_device_buffer((size_t)(ngroups + 2) * 8, ctx.device);
  }
}

// Stage 5, the main kernel: MAX_OUT fixed-width columns per pass.  Only the first pass evaluates the predicate (writing the
// selection bitmap when anything follows up) and is timed.
void FilterCall::launch_main() {
  for (int ci : fixed_cols) {   // output capacity = mask_len rows
    Column& o = out.cols[ci];
    auto vb = make_device_buffer((size_t)mask_len * o.width + 16, ctx.device);
    o.values = (const uint8_t*)vb->ptr; o.owned.push_back(vb);
    ctx.stats.bytes_read_alg += mask_len * o.width;
  }
  // predicate inputs that are not output columns cannot occur for filter_record (SELECT * semantics):
  // every referenced column is also copied, so it is counted once above.
  Scratch* ds = dev_scratch(ctx);
  const int gcap = grid_cap(ctx, tile_kind);
  size_t next_fixed = 0;
  bool first = true;
  do {
    FilterParams p{};
    p.nrows = mask_len;
    bind_scratch(p, ctx);
    p.sel_mask = (first && need_followup) ? (u64*)sel_mask->ptr : nullptr;
    p.grp_base = (first && need_followup) ? (u64*)grp_base->ptr : nullptr;
    if (first) fill_refs(p.pb, fp.lw, *fp.rec, str_bufs);
    else {   // later passes re-read the selection bitmap as a Boolean column
      p.pb.n_instr = 1; p.pb.n_refs = 1;
      Instr in{}; in.op = OP_LOAD; in.type = T_BOOL; in.src_kind = SRC_COL; in.src_type = T_BOOL; in.src_idx = 0;
      p.pb.prog[0] = in;
      ColRef r{}; r.values = sel_mask->ptr; r.type = T_BOOL; p.pb.refs[0] = r;
    }
    std::vector<int> launch_cols;
    while (next_fixed < fixed_cols.size() && (int)launch_cols.size() < MAX_OUT) launch_cols.push_back(fixed_cols[next_fixed++]);
    // narrow predicate input columns stay on chip between the predicate and copy phases (placed last)
    p.n_stash = 0;
    if (first) pick_stash(p, ctx, fp.lw, rec.cols, launch_cols, tile_kind);
    fill_outs(p, launch_cols, rec.cols, [&](int ci) { return rec.cols[ci].values0(); }, [&](int ci) { return (void*)out.cols[ci].values; });
    if (first) {   // the Utf8Fold slots: output offsets / bytes at input capacity, a byte-scan status word per tile
      for (size_t u = 0; u < fold_cols.size(); ++u) {
        const Column& c = rec.cols[fold_cols[u]];
        Column& o = out.cols[fold_cols[u]];
        auto offb = make_device_buffer((size_t)(mask_len + 2) * 4, ctx.device);
        auto db = make_device_buffer((size_t)fold_cap[u] + 16, ctx.device);
        auto st = make_device_buffer((size_t)(ntiles + 1) * 8, ctx.device);
        check_hip(hipMemsetAsync(st->ptr, 0, (size_t)(ntiles + 1) * 8, ctx.stream), "memset byte-scan status");
        fold_status.push_back(st);
        Utf8Fold& u8 = p.utf8[u];
        u8.in_offsets = (const int32_t*)c.values0(); u8.in_data = c.data;
        u8.out_offsets = (int32_t*)offb->ptr; u8.out_data = fold_data[u] ? (uint8_t*)db->ptr : nullptr;
        u8.status = (u64*)st->ptr; u8.total_bytes = &dev_scratch(ctx)->fold_bytes[u];
        o.values = (const uint8_t*)offb->ptr; o.owned.push_back(offb);
        o.data = (const uint8_t*)db->ptr; o.owned.push_back(db);
        ctx.stats.bytes_read_alg += mask_len * 8;   // offsets, by both phases (as the separate Utf8 pass counts them)
      }
      p.n_utf8 = (int32_t)fold_cols.size();
      clear_scratch(ctx, ntiles);
    } else {
      check_hip(hipMemsetAsync(ds, 0, kPerPass, ctx.stream), "memset scratch");
      check_hip(hipMemsetAsync(dev_status(ctx), 0, (size_t)(ntiles + 1) * 8, ctx.stream), "memset status");
    }
    const int kind = first ? tile_kind : (tile_kind == 2 ? 1 : tile_kind);   // kinds 1 and 2 share a tile size
    if (first) kernel_span_begin(ctx);
    launch_tiles(ctx, p, mask_len, tile_rows, gcap, [&](bool partial, int grid, bool tail) {
      if (tail) p.ticket = &ds->ticket2;
      check_hip(launch_filter(p, kind, partial, grid, ctx.stream), tail ? "launch filter_fused_kernel (tail)" : "launch filter_fused_kernel");
    });
    if (first) kernel_span_end(ctx);
    for (size_t u = 0; u < fold_cols.size(); ++u) {   // long folded strings: their bytes (first pass only)
      if (!first || fold_data[u]) continue;
      Utf8Params up{};
      up.nrows = mask_len; up.sel_mask = (const u64*)sel_mask->ptr; up.grp_base = (const u64*)grp_base->ptr;
      up.in_offsets = p.utf8[u].in_offsets; up.in_data = p.utf8[u].in_data;
      up.out_offsets = p.utf8[u].out_offsets; up.out_data = (uint8_t*)out.cols[fold_cols[u]].data;
      check_hip(launch_utf8_copy(up, (int)std::min<int64_t>((ngroups + 3) / 4, (int64_t)ctx.num_cus * 16), ctx.stream), "launch utf8_copy_kernel");
      ++ctx.stats.launches;
    }
    first = false;
  } while (next_fixed < fixed_cols.size());
}

// Stage 6, the row count; the split bounds and the first follow-up round's Utf8 byte spans ride on its read-back
void FilterCall::read_main() {
  BufferPtr split_dev;
  if (split && !split->starts.empty()) {
    const size_t n = split->starts.size();
    split_dev = make_device_buffer(n * 16 + 16, ctx.device);
    check_hip(hipMemcpyAsync(split_dev->ptr, split->starts.data(), n * 8, hipMemcpyHostToDevice, ctx.stream), "upload split rows");
    SplitBoundsParams sp{};
    sp.nrows = mask_len; sp.n = (int64_t)n; sp.starts = (const int64_t*)split_dev->ptr;
    sp.sel_mask = (const u64*)sel_mask->ptr; sp.grp_base = (const u64*)grp_base->ptr; sp.total = &dev_scratch(ctx)->total;
    sp.out = (u64*)((uint8_t*)split_dev->ptr + n * 8);
    check_hip(launch_split_bounds(sp, ctx.stream), "launch split_bounds_kernel");
    split->bounds.assign(n, 0);
    check_hip(hipMemcpyAsync(split->bounds.data(), sp.out, n * 8, hipMemcpyDeviceToHost, ctx.stream), "read back split bounds");
  }
  gather_utf8_ends(0, std::min(kUtf8PerRound, utf8_cols.size()));
  const Scratch* hs = read_scratch(ctx);
  ctx.stats.kernel_ns += kernel_span_ns(ctx);
  if (hs->err != ERR_NONE) throw_device_error(hs->err);
  total = out.nrows = (int64_t)hs->total;
  ctx.stats.rows_out = total; ctx.stats.tiles = ntiles;
  for (int ci : fixed_cols) { out.cols[ci].length = total; ctx.stats.bytes_written_alg += total * out.cols[ci].width; }
  for (size_t u = 0; u < fold_cols.size(); ++u) {
    Column& o = out.cols[fold_cols[u]];
    o.length = total; o.data_bytes = (int64_t)hs->fold_bytes[u];
    ctx.stats.bytes_read_alg += o.data_bytes; ctx.stats.bytes_written_alg += (total + 1) * 4 + o.data_bytes;
  }
}

// Stage 7, the follow-up kernels: Boolean and validity bitmaps, the Utf8 columns the main kernel did not take.  They report
// through the scratch header, kNullPerRound / kUtf8PerRound per round; wider batches take more rounds (one read-back each).
void FilterCall::follow_ups() {
  if (!need_followup) return;
  Scratch* ds = dev_scratch(ctx);
  const Scratch* hs = (const Scratch*)ctx.pinned.ptr;   // (read back by read_main)
  const int fgrid = (int)std::min<int64_t>((ngroups + 31) / 32, (int64_t)ctx.num_cus * 8);
  const size_t words = (size_t)(total + 31) / 32 + 2;
  auto bit_compact = [&](const uint8_t* in_bits, int64_t bit_off, u64* zero_counter) {
    auto ob = make_device_buffer(words * 4 + 8, ctx.device);
    check_hip(hipMemsetAsync(ob->ptr, 0, words * 4 + 8, ctx.stream), "memset bits");
    BitCompactParams bp{};
    bp.nrows = mask_len; bp.sel_mask = (const u64*)sel_mask->ptr; bp.grp_base = (const u64*)grp_base->ptr;
    bp.in_bits = in_bits; bp.in_bit_offset = bit_off; bp.out_bits = (uint32_t*)ob->ptr; bp.zero_count = zero_counter;
    check_hip(launch_bit_compact(bp, std::max(1, fgrid), ctx.stream), "launch bit_compact_kernel");
    ++ctx.stats.launches;
    return ob;
  };
  for (int ci : bool_cols) {
    auto ob = bit_compact(rec.cols[ci].values, rec.cols[ci].offset, nullptr);
    out.cols[ci].values = (const uint8_t*)ob->ptr; out.cols[ci].owned.push_back(ob); out.cols[ci].length = total;
  }
  std::vector<BufferPtr> byte_status(utf8_cols.size());
  size_t n0 = 0, u0 = 0;
  for (bool first_round = true; first_round || n0 < nullable_cols.size() || u0 < utf8_cols.size(); first_round = false) {
    const size_t n1 = std::min(n0 + kNullPerRound, nullable_cols.size()), u1 = std::min(u0 + kUtf8PerRound, utf8_cols.size());
    if (!first_round) {   // fresh counters, and the byte spans of this round's Utf8 columns
      check_hip(hipMemsetAsync(ds->counters, 0, sizeof(ds->counters), ctx.stream), "memset counters");
      if (u1 > u0) {
        gather_utf8_ends(u0, u1);
        hs = read_scratch(ctx);
      }
    }
    for (size_t k = n0; k < n1; ++k) {
      const int ci = nullable_cols[k];
      auto ob = bit_compact(rec.cols[ci].validity, rec.cols[ci].offset, &ds->counters[k - n0]);
      out.cols[ci].validity = (const uint8_t*)ob->ptr; out.cols[ci].owned.push_back(ob);
    }
    // Short strings: one fused pass (new offsets + bytes, 8192-row tiles).  Long strings: offsets pass (2048-row
    // tiles) then a copy pass with one wave per 64 rows, which spreads the byte copies over far more waves.
    for (size_t k = u0; k < u1; ++k) {
      const int ci = utf8_cols[k];
      const Column& c = rec.cols[ci];
      Column& o = out.cols[ci];
      const int64_t cap = (int64_t)hs->utf8_ends[2 * (k - u0) + 1] - hs->utf8_ends[2 * (k - u0)];
      const bool fused = cap <= mask_len * 24;
      const int64_t utile_rows = fused ? 8192 : 2048;
      const int64_t utiles = (mask_len + utile_rows - 1) / utile_rows;
      auto offb = make_device_buffer((size_t)(total + 2) * 4, ctx.device);
      auto db = make_device_buffer((size_t)cap + 16, ctx.device);
      byte_status[k] = make_device_buffer((size_t)(utiles + 64) * 8 + 16, ctx.device);
      check_hip(hipMemsetAsync(byte_status[k]->ptr, 0, (size_t)(utiles + 64) * 8 + 16, ctx.stream), "memset");
      Utf8Params up{};
      up.nrows = mask_len; up.sel_mask = (const u64*)sel_mask->ptr; up.grp_base = (const u64*)grp_base->ptr;
      up.in_offsets = (const int32_t*)c.values0(); up.in_data = c.data;
      up.out_offsets = (int32_t*)offb->ptr; up.out_data = (uint8_t*)db->ptr;
      up.byte_status = (u64*)byte_status[k]->ptr;
      up.ticket = (uint32_t*)((uint8_t*)byte_status[k]->ptr + (size_t)(utiles + 64) * 8);
      up.total_bytes = &ds->counters[kNullPerRound + (k - u0)];   // counters[16..23]: byte totals
      up.rows_out = total;
      if (fused) {
        check_hip(launch_utf8_filter(up, (int)std::min<int64_t>(utiles, (int64_t)ctx.num_cus * 2), ctx.stream), "launch utf8_filter_kernel");
        ++ctx.stats.launches;
      } else {
        check_hip(launch_utf8_offsets(up, (int)std::min<int64_t>(utiles, (int64_t)ctx.num_cus * 8), ctx.stream), "launch utf8_offsets_kernel");
        check_hip(launch_utf8_copy(up, (int)std::min<int64_t>((ngroups + 3) / 4, (int64_t)ctx.num_cus * 16), ctx.stream), "launch utf8_copy_kernel");
        ctx.stats.launches += 2;
      }
      o.values = (const uint8_t*)offb->ptr; o.owned.push_back(offb); o.length = total;
      o.data = (const uint8_t*)db->ptr; o.owned.push_back(db);
    }
    hs = read_scratch(ctx);
    for (size_t k = n0; k < n1; ++k) {
      Column& o = out.cols[nullable_cols[k]];
      o.null_count = (int64_t)hs->counters[k - n0];
      if (o.null_count == 0) o.validity = nullptr;   // arrow drops an all-valid null buffer
    }
    for (size_t k = u0; k < u1; ++k) {   // offsets read by both passes, selected bytes read and written, new offsets
      Column& o = out.cols[utf8_cols[k]];
      o.data_bytes = (int64_t)hs->counters[kNullPerRound + (k - u0)];
      ctx.stats.bytes_read_alg += mask_len * 8 + o.data_bytes; ctx.stats.bytes_written_alg += (total + 1) * 4 + o.data_bytes;
    }
    n0 = n1; u0 = u1;
  }
}

// What both host fast paths take: every column fixed-width (not Boolean / Utf8) and free of nulls; a bitmap whose null count
// is unknown (null_count < 0) is counted.  `row_bytes`: optional, the bytes of one row.
bool plain_host_columns(const Batch& rec, int64_t* row_bytes = nullptr) {
  int64_t bytes = 0;
  for (const Column& c : rec.cols) {
    if (c.type == T_BOOL || c.type == T_UTF8 || c.width <= 0) return false;
    if (c.validity && c.null_count != 0 && (c.null_count > 0 || count_nulls_host(c.validity, c.offset, c.length) != 0)) return false;
    bytes += c.width;
  }
  if (row_bytes) *row_bytes = bytes;
  return true;
}

}  // namespace

// =================================================================================================
// shared with group.cpp, group_concat.cpp and project.cpp (engine_internal.hpp)
// =================================================================================================
void fill_refs(ProgramBlock& pb, const Lowered& lw, const Batch& rec, const std::vector<BufferPtr>& str_bufs) {
  pb.n_instr = (int32_t)lw.prog.size();
  pb.n_refs = (int32_t)lw.refs.size();
  pb.fast_kind = FAST_NONE;
  for (size_t i = 0; i < lw.prog.size(); ++i) pb.prog[i] = lw.prog[i];
  // Programs over non-null 32-bit columns are pre-decoded for the FASTK kernels (device_program.h); among them the shape
  // [LOAD col:T] [CMP literal] on a column of exactly the compare type has its own even leaner device path.
  if (encode_fast_uops(pb, lw, rec)) {
    pb.fast_kind = FAST_UOPS;
    if (lw.prog.size() == 2 && lw.refs.size() == 1 && lw.prog[0].op == OP_LOAD && lw.prog[0].src_kind == SRC_COL &&
        lw.prog[0].src_type == lw.prog[0].type && lw.prog[1].op >= OP_EQ && lw.prog[1].op <= OP_GE &&
        lw.prog[1].src_kind == SRC_CONST && lw.prog[1].type == lw.prog[0].type)
      pb.fast_kind = FAST_CMP_CONST;
  }
  for (size_t i = 0; i < lw.refs.size(); ++i) {
    const Column& c = rec.cols[lw.refs[i]];
    ColRef r{};
    r.values = c.values0();
    r.validity = c.live_validity();
    r.data = c.data;
    r.validity_bit_offset = c.offset;
    r.bool_bit_offset = c.offset;
    // a temporal column inside a program is one side of a same-type comparison: its values ARE Int32 / Int64 (plan.cpp)
    r.type = c.type == T_FIXED_OPAQUE ? (c.width == 4 ? T_I32 : T_I64) : c.type;
    pb.refs[i] = r;
  }
  for (size_t i = 0; i < lw.strs.size(); ++i) { pb.strs[i].bytes = (const uint8_t*)str_bufs[i]->ptr; pb.strs[i].len = (int64_t)lw.strs[i].size(); }
}

// A Utf8 literal queued into device memory.  Both the string and the buffer must outlive the next wait for the stream.
BufferPtr upload_literal(Context& ctx, const std::string& s) {
  auto b = make_device_buffer(s.size() + 16, ctx.device);
  if (!s.empty()) check_hip(hipMemcpyAsync(b->ptr, s.data(), s.size(), hipMemcpyHostToDevice, ctx.stream), "upload string literal");
  return b;
}
std::vector<BufferPtr> upload_strings(Context& ctx, const Lowered& lw) {
  std::vector<BufferPtr> out;
  for (const auto& s : lw.strs) out.push_back(upload_literal(ctx, s));
  // literals live on the host stack of the caller: make the copies land before returning to it
  if (!out.empty()) check_hip(hipStreamSynchronize(ctx.stream), "sync");
  return out;
}

[[noreturn]] void throw_device_error(unsigned long long stored) {
  const unsigned long long err = ~stored;   // the device keeps the complement (see ERR_NONE)
  const int code = (int)(err & 0xff);
  const long long row = (long long)((err >> 8) & ((1ULL << 48) - 1));
  if (code == DE_DIV_ZERO) throw ChqError{CHQ_ERR_ARROW_DIVIDE_BY_ZERO, "Divide by zero error (row " + std::to_string(row) + ")"};
  throw ChqError{CHQ_ERR_ARROW_ARITHMETIC_OVERFLOW, "Overflow happened on row " + std::to_string(row)};
}

int pick_tile_kind(const Context& ctx, const Lowered& lw, int64_t rows) {
  if (lw.wide || lw.num_temps > 0) return 2;
  if (ctx.opt_tile_kind >= 0) return (int)ctx.opt_tile_kind;
  return rows >= (1 << 18) ? 0 : 1;
}

// Up to `slots` narrow predicate input columns stay on chip between the predicate and copy phases (device_program.h:
// FilterParams::stash_refs); they move to the end of the launch's column order, slot k <-> the k-th of them.
void pick_stash(FilterParams& p, const Context& ctx, const Lowered& lw, const std::vector<Column>& cols, std::vector<int>& launch_cols, int tile_kind) {
  const int slots = std::min<int>(kStashSlots[tile_kind], ctx.opt_stash < 0 ? MAX_STASH : (int)ctx.opt_stash);
  p.n_stash = 0;
  std::vector<int> chosen;
  for (size_t r = 0; r < lw.refs.size() && r < 127 && p.n_stash < slots; ++r) {
    const int ci = lw.refs[r];
    if ((size_t)ci >= cols.size() || !stashable(cols[ci])) continue;   // (a temporary column is not an output column)
    if (std::find(chosen.begin(), chosen.end(), ci) != chosen.end()) continue;
    auto it = std::find(launch_cols.begin(), launch_cols.end(), ci);
    if (it == launch_cols.end()) continue;
    launch_cols.erase(it); launch_cols.push_back(ci);
    chosen.push_back(ci);
    p.stash_refs[p.n_stash++] = (int8_t)r;
  }
}

// The reference's error order: data-dependent errors of subtrees evaluated before a static error take precedence over it
void throw_pending(Context& ctx, const Batch& rec, const std::vector<PlanColumn>& pcols, const TypedExpr& te) {
  if (rec.nrows > 0) {
    std::vector<TypedExpr> subs;
    for (int r : te.validate_roots) { TypedExpr s; s.nodes = te.nodes; s.root = r; subs.push_back(std::move(s)); }
    std::vector<const TypedExpr*> ptrs;
    for (auto& s : subs) ptrs.push_back(&s);
    (void)evaluate_dense(ctx, rec, pcols, ptrs);   // throws the data-dependent error if there is one
  }
  throw ChqError{te.pending_code, te.pending_msg};
}
// type_expr in that order
TypedExpr typed(Context& ctx, const Batch& rec, const std::vector<PlanColumn>& pcols, const Expr& expr) {
  TypedExpr te = type_expr(expr, pcols, rec.nrows, ctx.opt_enable_minus);
  if (te.pending_code) throw_pending(ctx, rec, pcols, te);
  return te;
}

// what the one-launch paths filter with: no pending error, a Boolean result, not a literal-only (length-1) mask
bool is_row_predicate(const TypedExpr& te) {
  if (te.pending_code) return false;
  const Node& root = te.at(te.root);
  return root.type == T_BOOL && !root.len1;
}

Column empty_like(const Column& c) {
  Column o;
  o.name = c.name; o.format = c.format; o.type = c.type; o.width = c.width; o.nullable = c.nullable;
  return o;
}

// ---- the uniform-length Utf8 rewrite (filter_record and the group path) -------------------------------------------------
// A Utf8 column qualifies when it has no bitmap that may hold nulls (the rewrite zeroes the Arrow offset a bitmap is read
// at), all its values have one length L in {1, 2, 4, 8, 16} (whole values per lane) and rows x L fits int32 offsets.
// Asked with L = 1 before the lengths are known.
bool uniform_utf8_ok(bool may_hold_nulls, int64_t rows, int64_t L) {
  return !may_hold_nulls && (L == 1 || L == 2 || L == 4 || L == 8 || L == 16) && rows * L < (1ll << 31) - 64;
}
// The rebuild: the fixed-width (w:L) output of such a column back to Utf8 with the schema of `like` -- its values become
// the bytes, and the offsets 0, L, 2 L, ... are written where the column lives
Column uniform_to_utf8(Context& ctx, Column&& fixed, const Column& like, int64_t rows, bool on_device) {
  const int32_t L = fixed.width;
  BufferPtr ob;
  if (on_device) {
    ob = make_device_buffer((size_t)(rows + 1) * 4 + 16, ctx.device);
    IotaOffsetsParams ip{(int32_t*)ob->ptr, rows + 1, L, 0};
    check_hip(launch_iota_offsets(ip, ctx.stream), "launch iota_offsets_kernel");
  } else {
    ob = make_host_buffer((size_t)(rows + 1) * 4 + 16);
    int32_t* o = (int32_t*)ob->ptr;
    for (int64_t r = 0; r <= rows; ++r) o[r] = (int32_t)(r * L);
  }
  Column u = empty_like(like);
  u.length = rows; u.null_count = 0; u.offset = 0;
  u.data = (const uint8_t*)fixed.values0(); u.data_bytes = rows * (int64_t)L;
  u.values = (const uint8_t*)ob->ptr;
  u.owned = std::move(fixed.owned); u.owned.push_back(ob);
  ctx.stats.bytes_written_alg += (rows + 1) * 4;
  return u;
}

// =================================================================================================
// filter_record
// =================================================================================================
Batch filter_record(Context& ctx, const Batch& rec, const std::vector<PlanColumn>& pcols, const Expr& expr, SplitRequest* split) {
  FilterProgram fp;
  type_filter(ctx, rec, pcols, expr, fp);
  Batch res;
  if (uniform_detour(ctx, rec, pcols, expr, split, fp, &res)) return res;
  ctx.stats = chq_call_stats{};
  ctx.stats.rows_in = rec.nrows;
  if (fp.mask_len == 0) return empty_filter_result(ctx, rec);
  FilterCall f(ctx, rec, fp, split);
  f.plan_fold();
  f.launch_main();
  f.read_main();
  f.follow_ups();
  for (Column& o : f.out.cols) o.length = f.total;
  return std::move(f.out);
}

// =================================================================================================
// filter_record_large_host: one LARGE host batch in, one host batch out.  The general path is three serial steps -- upload
// everything (10.6 ms for 50 M rows x 12 B), one 0.25 ms kernel, download everything (12.1 ms) -- on a link that is full
// duplex.  Here the batch is cut into chunks of a few million rows: chunk k is filtered by the ordinary single-batch path
// (so every semantic detail, the error order included, is the single-batch path's), its survivors start their way down to
// the host on a second stream, and the host thread moves on to uploading chunk k+1 while that download runs: uploads and
// downloads overlap, the call approaches max(upload, download) instead of their sum.  Fixed-width non-null columns and a
// non-literal predicate; anything else takes the general path.
// =================================================================================================
bool filter_record_large_host(Context& ctx, const Batch& rec, const chq_table_aliases* aliases, const Expr& expr, Batch* result) {
  const int64_t nrows = rec.nrows;
  const size_t ncols = rec.cols.size();
  if (!ctx.opt_large_host || rec.on_device || nrows < ctx.opt_large_host_rows || ncols == 0 || (int)ncols > MAX_OUT) return false;
  int64_t row_bytes = 0;
  if (!plain_host_columns(rec, &row_bytes)) return false;
  const std::vector<PlanColumn> pcols = plan_columns(rec, aliases);
  try {
    if (!is_row_predicate(type_expr(expr, pcols, nrows, ctx.opt_enable_minus))) return false;
  } catch (const ChqError&) {
    return false;   // the general path reports it
  }
  // chunk: about 64 MB of input, a whole number of 16 384-row tiles
  int64_t chunk = std::max<int64_t>(1 << 20, ((int64_t)64 << 20) / std::max<int64_t>(1, row_bytes));
  if (ctx.opt_large_host_chunk > 0) chunk = ctx.opt_large_host_chunk;
  chunk = (chunk + 16383) / 16384 * 16384;
  ensure_aux_streams(ctx);   // (created once per context; also used by the Parquet scan)
  const hipStream_t down = ctx.aux[0];
  Batch out;
  out.on_device = false; out.device_id = -1;
  std::vector<BufferPtr> host_cols;
  for (const Column& c : rec.cols) {
    Column o = empty_like(c);
    auto hb = make_host_buffer((size_t)nrows * c.width + 64);
    o.values = (const uint8_t*)hb->ptr; o.owned.push_back(hb);
    host_cols.push_back(hb);
    out.cols.push_back(std::move(o));
  }
  // Host memory on both ends is pageable, so a copy call keeps its calling thread busy until the bytes have moved: the
  // downloads get a thread of their own.  It takes finished chunks off a queue (at most three wait: that bounds the HBM
  // held), copies their survivors to their place in the result and only then lets the chunk's buffers go back to the pool.
  struct Job { Batch dev_in, dev_out; int64_t base = 0; };
  std::mutex qm; std::condition_variable qcv;
  std::deque<Job> queue;
  bool closed = false;
  std::exception_ptr dl_error;
  const int device = ctx.device;
  std::thread downloader([&] {
    try {
      check_hip(hipSetDevice(device), "hipSetDevice");
      while (true) {
        Job job;
        {
          std::unique_lock<std::mutex> l(qm);
          qcv.wait(l, [&] { return closed || !queue.empty(); });
          if (queue.empty()) return;
          job = std::move(queue.front());
        }
        for (size_t i = 0; i < ncols; ++i) {
          const Column& rc = job.dev_out.cols[i];
          if (job.dev_out.nrows) check_hip(hipMemcpyAsync((uint8_t*)host_cols[i]->ptr + (size_t)job.base * rc.width, rc.values0(),
                                                         (size_t)job.dev_out.nrows * rc.width, hipMemcpyDeviceToHost, down), "download survivors");
        }
        check_hip(hipStreamSynchronize(down), "hipStreamSynchronize");
        { std::lock_guard<std::mutex> l(qm); queue.pop_front(); }   // (popped only now: the queue length bounds chunks in flight)
        qcv.notify_all();
      }
    } catch (...) {
      std::lock_guard<std::mutex> l(qm);
      dl_error = std::current_exception();
      queue.clear();
      qcv.notify_all();
    }
  });
  auto finish = [&] { { std::lock_guard<std::mutex> l(qm); closed = true; } qcv.notify_all(); if (downloader.joinable()) downloader.join(); };
  chq_call_stats acc{};
  int64_t total = 0;
  try {
    for (int64_t r0 = 0; r0 < nrows; r0 += chunk) {
      const int64_t n = std::min(chunk, nrows - r0);
      Batch view;
      view.nrows = n; view.on_device = false; view.device_id = -1;
      for (const Column& c : rec.cols) { Column v = c; v.offset = c.offset + r0; v.length = n; v.validity = nullptr; v.null_count = 0; view.cols.push_back(std::move(v)); }
      Batch dev = to_device(ctx, view);                                        // upload: this thread is busy with it
      Batch res = filter_record(ctx, dev, plan_columns(dev, aliases), expr);   // kernel + row count (synchronises ctx.stream)
      add_stats(acc, ctx.stats);
      Job job; job.base = total; total += res.nrows; job.dev_in = std::move(dev); job.dev_out = std::move(res);
      std::unique_lock<std::mutex> l(qm);
      qcv.wait(l, [&] { return dl_error || queue.size() < 3; });
      if (dl_error) break;
      queue.push_back(std::move(job));
      l.unlock();
      qcv.notify_all();
    }
  } catch (...) {
    finish();
    throw;
  }
  finish();
  if (dl_error) std::rethrow_exception(dl_error);
  out.nrows = total;
  for (Column& o : out.cols) { o.length = total; o.null_count = 0; o.validity = nullptr; }
  acc.rows_in = nrows; acc.rows_out = total;
  ctx.stats = acc;
  *result = std::move(out);
  return true;
}

// =================================================================================================
// filter_record_small_host: the reference's own calling pattern -- one 10 000-row host batch in, one host batch out --
// costs three pageable uploads, three pageable downloads (each of them synchronous) and two stream synchronisations on
// the general path: about 100 us, i.e. no faster than the CPU.  Here the columns are packed into ONE pinned block,
// uploaded with one asynchronous copy, the outputs are written into one device block at input capacity and come back
// with one asynchronous copy together with the row count: one synchronisation per call.
// =================================================================================================
bool filter_record_small_host(Context& ctx, const Batch& rec, const chq_table_aliases* aliases, const Expr& expr, Batch* result) {
  const int64_t nrows = rec.nrows;
  const size_t ncols = rec.cols.size();
  if (!ctx.opt_small_host || rec.on_device || nrows < 2 || nrows > (1 << 18) || ncols == 0 || (int)ncols > MAX_OUT) return false;
  if (!plain_host_columns(rec)) return false;
  constexpr size_t kAlign = 256;
  std::vector<size_t> at(ncols + 1, 0);
  for (size_t i = 0; i < ncols; ++i) at[i + 1] = at[i] + ((size_t)nrows * rec.cols[i].width + kAlign - 1) / kAlign * kAlign;
  const size_t block = at[ncols];
  if (block > ((size_t)8 << 20)) return false;
  const std::vector<PlanColumn> pcols = plan_columns(rec, aliases);
  Lowered lw;
  try {
    TypedExpr te = type_expr(expr, pcols, nrows, ctx.opt_enable_minus);
    if (!is_row_predicate(te)) return false;
    lower_expr(te, te.root, pcols, lw);
  } catch (const ChqError&) {
    return false;   // the general path reports it
  }
  if (!lw.strs.empty()) return false;

  if (ctx.pinned_io.bytes < 2 * block + 64) {
    const size_t cap = std::max<size_t>(2 * block + 64, (size_t)1 << 20);
    ctx.dev_io = make_device_buffer(cap, ctx.device);   // may throw: the pinned half grows (and records its capacity) only after it
    ctx.pinned_io.reserve(2 * block + 64, cap, "hipHostMalloc (small host path)");
  }
  uint8_t* h_in = (uint8_t*)ctx.pinned_io.ptr; uint8_t* h_out = h_in + block;
  uint8_t* d_in = (uint8_t*)ctx.dev_io->ptr; uint8_t* d_out = d_in + block;
  for (size_t i = 0; i < ncols; ++i) memcpy(h_in + at[i], rec.cols[i].values0(), (size_t)nrows * rec.cols[i].width);
  check_hip(hipMemcpyAsync(d_in, h_in, block, hipMemcpyHostToDevice, ctx.stream), "upload packed batch");

  const int tile_kind = (lw.wide || lw.num_temps > 0) ? 2 : 1;
  const int64_t tile_rows = kTileRows[tile_kind];
  const int64_t ntiles = (nrows + tile_rows - 1) / tile_rows;
  ensure_scratch(ctx, ntiles);

  // a view of the batch whose columns live in the device block (what the program's column refs resolve against)
  Batch dev;
  dev.nrows = nrows; dev.on_device = true; dev.device_id = ctx.device;
  for (size_t i = 0; i < ncols; ++i) {
    Column c = empty_like(rec.cols[i]);
    c.length = nrows; c.values = d_in + at[i];
    dev.cols.push_back(std::move(c));
  }
  FilterParams p{};
  p.nrows = nrows; p.tile_begin = 0; p.tile_end = ntiles;
  bind_scratch(p, ctx);
  fill_refs(p.pb, lw, dev, {});
  std::vector<int> launch_cols;
  for (size_t i = 0; i < ncols; ++i) launch_cols.push_back((int)i);
  pick_stash(p, ctx, lw, rec.cols, launch_cols, tile_kind);
  fill_outs(p, launch_cols, rec.cols, [&](int ci) { return d_in + at[ci]; }, [&](int ci) { return d_out + at[ci]; });
  ctx.stats = chq_call_stats{};
  ctx.stats.rows_in = nrows; ctx.stats.tiles = ntiles; ctx.stats.launches = 1;
  clear_scratch(ctx, ntiles);
  const int gcap = ctx.num_cus * kGridPerCu[tile_kind];   // (not grid_cap: this path has never read `grid_per_cu`)
  check_hip(launch_filter(p, tile_kind, true, (int)std::min<int64_t>(ntiles, gcap), ctx.stream), "launch filter_fused_kernel (small host batch)");
  check_hip(hipMemcpyAsync(h_out, d_out, block, hipMemcpyDeviceToHost, ctx.stream), "download packed result");
  const Scratch* hs = read_scratch(ctx);
  if (hs->err != ERR_NONE) return false;   // the general path reports the error
  const int64_t total = (int64_t)hs->total;
  Batch out;
  out.on_device = false; out.device_id = -1; out.nrows = total;
  for (size_t i = 0; i < ncols; ++i) {
    Column o = empty_like(rec.cols[i]);
    auto hb = make_host_buffer((size_t)total * o.width + 16);
    if (total) memcpy(hb->ptr, h_out + at[i], (size_t)total * o.width);
    o.values = (const uint8_t*)hb->ptr; o.length = total; o.owned.push_back(hb);
    ctx.stats.bytes_read_alg += nrows * o.width; ctx.stats.bytes_written_alg += total * o.width;
    out.cols.push_back(std::move(o));
  }
  ctx.stats.rows_out = total;
  *result = std::move(out);
  return true;
}

}  // namespace chq
