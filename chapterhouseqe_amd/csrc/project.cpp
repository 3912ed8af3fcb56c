// project.cpp -- dense evaluation of typed expressions, compute_value, project_record, the fused filter + project pass, the
// host projection path and describe_plan.  Reference map: project_record = RU/record_projection.rs:16-76, compute_value =
// RU/compute_value.rs:57-344 (RU = src/handlers/operator_handler/operators/record_utils of the reference).
#include "engine_internal.hpp"

#include <cstdio>
#include <cstring>
#include <functional>

namespace chq {

// =================================================================================================
// project_record / compute_value
// =================================================================================================
namespace {

// deep copy of a column inside HBM (the reference Arc-clones; inputs here are only borrowed)
Column clone_device_column(Context& ctx, const Column& c) { return copy_column(ctx, c, Dir::D2D); }

Column scalar_column(Context& ctx, const Scalar& s, const std::string& name) {
  Column o;
  o.name = name; o.type = s.type; o.length = 1; o.null_count = 0; o.nullable = false;
  o.format = dtype_format(s.type); o.width = dtype_width(s.type);
  if (s.type == T_UTF8) {
    int32_t offs[2] = {0, (int32_t)s.str.size()};
    auto ob = make_device_buffer(16, ctx.device), db = make_device_buffer(s.str.size() + 16, ctx.device);
    check_hip(hipMemcpy(ob->ptr, offs, 8, hipMemcpyHostToDevice), "memcpy");
    if (!s.str.empty()) check_hip(hipMemcpy(db->ptr, s.str.data(), s.str.size(), hipMemcpyHostToDevice), "memcpy");
    o.values = (const uint8_t*)ob->ptr; o.data = (const uint8_t*)db->ptr; o.owned = {ob, db};
  } else {
    uint64_t bits[2] = {s.null ? 0 : s.bits, 0};   // second word: the validity bitmap of a NULL value
    auto vb = make_device_buffer(16, ctx.device);
    check_hip(hipMemcpy(vb->ptr, bits, 16, hipMemcpyHostToDevice), "memcpy");
    o.values = (const uint8_t*)vb->ptr; o.owned = {vb};
    if (s.null) { o.validity = (const uint8_t*)vb->ptr + 8; o.null_count = 1; o.nullable = true; }
  }
  return o;
}

struct ProjItem {   // one computed output of a launch
  int out_index;     // position in the output batch
  int null_slot;     // counter slot, -1 when the expression cannot produce nulls
};

bool subtree_can_null(const TypedExpr& t, int ni, const std::vector<PlanColumn>& cols) {
  const Node& n = t.at(ni);
  if (n.kind == Node::COL) return cols[n.col].has_nulls;
  if (n.kind == Node::CONST) return n.cval.null;
  if (n.kind == Node::ISNULL) return false;   // IS [NOT] NULL is never null
  bool r = (n.kind == Node::TOBOOL && n.from == T_UTF8) ||   // a bad spelling is NULL
           (n.kind == Node::XCAST && n.op != 0 && cast_can_fail(n.from, n.type));   // a failing TRY_CAST row too
  n.each_child([&](int c) { r = r || subtree_can_null(t, c, cols); });   // (a string function: null where an operand is)
  return r;
}

// an expression select item's name; `*unnamed_idx` counts the UNNAMED_EXPR items so far
std::string select_item_name(const chq_select_item& f, const Expr& e, size_t* unnamed_idx) {
  std::string name;
  if (f.kind == CHQ_ITEM_EXPR_WITH_ALIAS) name = f.alias ? f.alias : "";
  else if (e.kind == Expr::IDENT) name = e.text;                 // RU/record_projection.rs:41-48
  else name = "unnamed_" + std::to_string(*unnamed_idx);         // :49-53
  if (f.kind == CHQ_ITEM_UNNAMED_EXPR) ++*unnamed_idx;          // :58, counts identifiers too
  return name;
}

// the result of one compute_value call: a passthrough column, a literal-built length-1 array, or a program
struct Evaluated {
  enum Kind { PASSTHROUGH, SCALAR, COMPUTED } kind;
  int col = -1;
  Scalar value;
  TypedExpr typed;
  bool is_scalar = false;
};

Evaluated classify(Context& ctx, const Batch& rec, const Expr& e, const std::vector<PlanColumn>& pcols) {
  Evaluated ev;
  ev.typed = typed(ctx, rec, pcols, e);
  const Node& root = ev.typed.at(ev.typed.root);
  ev.is_scalar = root.is_scalar;
  if (root.kind == Node::COL) { ev.kind = Evaluated::PASSTHROUGH; ev.col = root.col; }
  else if (root.len1) { ev.kind = Evaluated::SCALAR; ev.value = fold_constant(ev.typed, ev.typed.root); }
  else ev.kind = Evaluated::COMPUTED;
  return ev;
}

}  // namespace

// Evaluate the expressions `exprs[k]` (typed trees) densely over `rec`; returns one column per expression.
std::vector<Column> evaluate_dense(Context& ctx, const Batch& rec, const std::vector<PlanColumn>& pcols,
                                   const std::vector<const TypedExpr*>& exprs) {
  const int64_t nrows = rec.nrows;
  std::vector<Column> results(exprs.size());
  for (size_t k = 0; k < exprs.size(); ++k) {
    const Node& root = exprs[k]->at(exprs[k]->root);
    Column& o = results[k];
    o.type = root.type; o.format = dtype_format(root.type); o.width = dtype_width(root.type); o.length = nrows;
    // (a Utf8 result is a string function's: fitting below turns it into a temporary column, which IS the result)
    // (.. or a CASE's, of any type)
    if (root.kind == Node::CASE && root.type == T_FIXED_OPAQUE) { o.format = pcols[(size_t)root.fmt_col].format; o.width = pcols[(size_t)root.fmt_col].width; }
    // (.. or an explicit cast's to Utf8)
    if (root.kind != Node::CASE && ((root.type == T_UTF8 && root.kind != Node::STRFN && root.kind != Node::XCAST) || root.type == T_FIXED_OPAQUE))
      throw ChqError{CHQ_ERR_NOT_SUPPORTED, std::string("expression result of type ") + dtype_name(root.type) + " is outside this build's scope"};
  }
  if (nrows == 0) {
    for (Column& o : results) {
      auto vb = make_device_buffer(16, ctx.device);
      o.values = (const uint8_t*)vb->ptr; o.owned.push_back(vb);
      if (o.type != T_UTF8) continue;
      auto db = make_device_buffer(16, ctx.device);   // offsets = {0}, no bytes
      check_hip(hipMemsetAsync(vb->ptr, 0, 16, ctx.stream), "memset");
      o.data = (const uint8_t*)db->ptr; o.data_bytes = 0; o.owned.push_back(db);
    }
    check_hip(hipStreamSynchronize(ctx.stream), "sync");
    return results;
  }
  ensure_scratch(ctx, 1);
  size_t k = 0;
  while (k < exprs.size()) {
    if (!lowers_alone(*exprs[k], exprs[k]->root, pcols)) {
      // too large for one program even alone: sub-trees become temporary columns first (fit_to_device), then the
      // rest is evaluated like any other expression
      Batch work; std::vector<PlanColumn> wcols; TypedExpr fitted;
      fit_to_device(ctx, rec, pcols, *exprs[k], work, wcols, fitted);
      if (fitted.at(fitted.root).kind == Node::COL) {   // a typed operation at the root: its temporary column is the result
        results[k] = work.cols[(size_t)fitted.at(fitted.root).col];
        results[k].name.clear();
        ++k;
        continue;
      }
      std::vector<const TypedExpr*> one{&fitted};
      Column c = std::move(evaluate_dense(ctx, work, wcols, one)[0]);
      results[k] = std::move(c);
      ++k;
      continue;
    }
    // pack as many expressions as fit the program limits into one launch
    Scratch* ds = dev_scratch(ctx);   // (looked up here: a nested call above may have replaced the block)
    Lowered lw;
    std::vector<ProjItem> items;
    int null_slots = 0;
    size_t k0 = k;
    for (; k < exprs.size() && (int)items.size() < MAX_PROJ; ++k) {
      Lowered trial = lw;
      try {
        lower_expr(*exprs[k], exprs[k]->root, pcols, trial);
        if ((int)trial.prog.size() + 1 > MAX_INSTR) throw ChqError{CHQ_ERR_NOT_SUPPORTED, "program too long"};
      } catch (const ChqError& e) {
        if (k == k0) throw;   // does not fit even alone
        break;
      }
      Instr st{}; st.op = OP_STORE; st.src_idx = (uint16_t)items.size(); st.src_kind = SRC_NONE;
      trial.prog.push_back(st);
      lw = std::move(trial);
      const bool can_null = subtree_can_null(*exprs[k], exprs[k]->root, pcols);
      if (can_null && null_slots >= 16) throw ChqError{CHQ_ERR_NOT_SUPPORTED, "too many nullable outputs in one projection"};
      items.push_back(ProjItem{(int)k, can_null ? null_slots++ : -1});
    }
    ProjectParams p{};
    p.nrows = nrows; p.err = &ds->err; p.n_proj = (int32_t)items.size();
    auto str_bufs = upload_strings(ctx, lw);
    fill_refs(p.pb, lw, rec, str_bufs);
    for (size_t i = 0; i < items.size(); ++i) {
      Column& o = results[items[i].out_index];
      const size_t vbytes = o.type == T_BOOL ? (size_t)((nrows + 63) / 64) * 8 + 16 : (size_t)nrows * o.width + 16;
      auto vb = make_device_buffer(vbytes, ctx.device);
      o.values = (const uint8_t*)vb->ptr; o.owned.push_back(vb);
      ProjOut po{};
      po.values = vb->ptr; po.type = o.type;
      if (items[i].null_slot >= 0) {
        auto nb = make_device_buffer((size_t)((nrows + 63) / 64) * 8 + 16, ctx.device);
        o.validity = (const uint8_t*)nb->ptr; o.owned.push_back(nb);
        po.validity = (u64*)nb->ptr; po.null_count = &ds->counters[items[i].null_slot];
      }
      p.outs[i] = po;
    }
    check_hip(hipMemsetAsync(ds, 0, sizeof(Scratch), ctx.stream), "memset scratch");
    const int tile_kind = pick_tile_kind(ctx, lw, nrows);
    launch_tiles(ctx, p, nrows, kTileRows[tile_kind], (int64_t)ctx.num_cus * (tile_kind == 0 ? 2 : 8), [&](bool partial, int grid, bool tail) {
      check_hip(launch_project(p, tile_kind, partial, grid, ctx.stream), tail ? "launch project_kernel (tail)" : "launch project_kernel");
    });
    const Scratch* hs = read_scratch(ctx);
    if (hs->err != ERR_NONE) {
      // Several expressions shared the launch and each numbers its nodes from zero, so the smallest (node, row) key may
      // belong to a later select item.  The reference evaluates the items one after the other: do the same to find
      // the error it would have reported.
      if (items.size() > 1) {
        for (const ProjItem& it : items) {
          std::vector<const TypedExpr*> one{exprs[it.out_index]};
          (void)evaluate_dense(ctx, rec, pcols, one);   // throws at the first failing item
        }
      }
      throw_device_error(hs->err);
    }
    for (const ProjItem& it : items) {
      Column& o = results[it.out_index];
      if (it.null_slot >= 0) { o.null_count = (int64_t)hs->counters[it.null_slot]; if (o.null_count == 0) o.validity = nullptr; }
    }
  }
  return results;
}

Column compute_value(Context& ctx, const Batch& rec, const std::vector<PlanColumn>& pcols, const Expr& expr, bool* is_scalar) {
  ctx.stats = chq_call_stats{};
  Evaluated ev = classify(ctx, rec, expr, pcols);
  if (is_scalar) *is_scalar = ev.is_scalar;
  Column out;
  switch (ev.kind) {
    case Evaluated::PASSTHROUGH: out = clone_device_column(ctx, rec.cols[ev.col]); check_hip(hipStreamSynchronize(ctx.stream), "sync"); break;
    case Evaluated::SCALAR: out = scalar_column(ctx, ev.value, ""); break;
    default: { std::vector<const TypedExpr*> v{&ev.typed}; out = std::move(evaluate_dense(ctx, rec, pcols, v)[0]); } break;
  }
  out.nullable = out.null_count > 0;
  return out;
}

Batch project_record(Context& ctx, const std::vector<chq_select_item>& fields, const Batch& rec,
                     const std::vector<PlanColumn>& pcols) {
  ctx.stats = chq_call_stats{};
  Batch out;
  out.on_device = true; out.device_id = ctx.device;
  std::vector<Evaluated> evs;            // computed items, evaluated together after the walk
  std::vector<int> computed_slot;        // output column index of each computed item
  std::vector<size_t> passthrough_slot;  // output column index of each identifier item
  size_t unnamed_idx = 0;
  auto evaluate_items = [&]() -> std::vector<Column> {   // the computed items so far, in one evaluation
    if (evs.empty()) return {};
    std::vector<const TypedExpr*> ptrs;
    for (auto& ev : evs) ptrs.push_back(&ev.typed);
    return evaluate_dense(ctx, rec, pcols, ptrs);
  };
  for (const chq_select_item& f : fields) {
    switch (f.kind) {
      case CHQ_ITEM_WILDCARD:   // RU/record_projection.rs:27-32
        for (const Column& c : rec.cols) out.cols.push_back(clone_device_column(ctx, c));
        break;
      case CHQ_ITEM_QUALIFIED_WILDCARD:
        (void)evaluate_items();
        throw ChqError{CHQ_ERR_PROJECT_NOT_IMPLEMENTED, "not implemented: SelectItem::QualifiedWildcard"};
      case CHQ_ITEM_UNNAMED_EXPR:
      case CHQ_ITEM_EXPR_WITH_ALIAS: {
        if (!f.expr) throw ChqError{CHQ_ERR_INVALID_HANDLE, "select item without expression"};
        const Expr& e = *(const Expr*)f.expr;
        Evaluated ev;
        try {
          ev = classify(ctx, rec, e, pcols);
        } catch (const ChqError&) {
          (void)evaluate_items();   // the reference evaluates the items in order: errors of earlier computed items come first
          throw;
        }
        const std::string name = select_item_name(f, e, &unnamed_idx);
        Column col;
        if (ev.kind == Evaluated::PASSTHROUGH) { col = clone_device_column(ctx, rec.cols[ev.col]); passthrough_slot.push_back(out.cols.size()); }
        else if (ev.kind == Evaluated::SCALAR) col = scalar_column(ctx, ev.value, name);
        else { computed_slot.push_back((int)out.cols.size()); evs.push_back(std::move(ev)); }
        col.name = name;
        out.cols.push_back(std::move(col));
      } break;
      default: throw ChqError{CHQ_ERR_INVALID_HANDLE, "unknown select item kind"};
    }
  }
  std::vector<Column> cols = evaluate_items();
  for (size_t i = 0; i < cols.size(); ++i) {
    std::string name = out.cols[computed_slot[i]].name;
    out.cols[computed_slot[i]] = std::move(cols[i]);
    out.cols[computed_slot[i]].name = name;
  }
  // an identifier over a view keeps the view's bitmap with its null count unknown (imported as "may have nulls"): count the
  // window's nulls, so that its nullability is the reference's null_count > 0 below
  std::vector<size_t> counted;
  for (size_t k : passthrough_slot) {
    Column& c = out.cols[k];
    if (c.validity && c.null_count != 0 && c.length == 0) { c.null_count = 0; c.validity = nullptr; }
    else if (c.validity && c.null_count != 0) counted.push_back(k);
  }
  BufferPtr d_valid;
  std::vector<unsigned long long> h_valid(counted.size(), 0);
  if (!counted.empty()) {
    d_valid = make_device_buffer(counted.size() * 8 + 16, ctx.device);
    check_hip(hipMemsetAsync(d_valid->ptr, 0, counted.size() * 8, ctx.stream), "memset");
    for (size_t j = 0; j < counted.size(); ++j) {
      const Column& c = out.cols[counted[j]];
      check_hip(launch_count_bits(c.validity, c.offset, c.length, (unsigned long long*)d_valid->ptr + j, ctx.stream), "launch count_bits_kernel");
    }
    check_hip(hipMemcpyAsync(h_valid.data(), d_valid->ptr, counted.size() * 8, hipMemcpyDeviceToHost, ctx.stream), "read back");
  }
  check_hip(hipStreamSynchronize(ctx.stream), "hipStreamSynchronize");
  for (size_t j = 0; j < counted.size(); ++j) {
    Column& c = out.cols[counted[j]];
    c.null_count = c.length - (int64_t)h_valid[j];
    if (c.null_count == 0) c.validity = nullptr;
  }
  // Field nullability: wildcard fields keep the schema flag; computed / identifier fields use
  // Array::is_nullable() = null_count > 0 (RU/record_projection.rs:45-47, 51-53, 62-66)
  {
    size_t k = 0;
    for (const chq_select_item& f : fields) {
      if (f.kind == CHQ_ITEM_WILDCARD) { k += rec.cols.size(); continue; }
      out.cols[k].nullable = out.cols[k].null_count > 0;
      ++k;
    }
  }
  // RecordBatch::try_new (RU/record_projection.rs:72-73)
  if (out.cols.empty()) throw ChqError{CHQ_ERR_ARROW_INVALID_ARGUMENT, "must either specify a row count or at least one column"};
  const int64_t len = out.cols[0].length;
  for (const Column& c : out.cols) {
    if (c.length != len) throw ChqError{CHQ_ERR_ARROW_INVALID_ARGUMENT, "all columns in a record batch must have the same length"};
    if (!c.nullable && c.null_count > 0)
      throw ChqError{CHQ_ERR_ARROW_INVALID_ARGUMENT, "Column '" + c.name + "' is declared as non-nullable but contains null values"};
  }
  out.nrows = len;
  return out;
}

// =================================================================================================
// filter_project_fused: filter_record + project_record in ONE pass when the inputs allow it.
// Returns false when the call is outside the fused kernel's scope or when the device flagged any error -- the caller
// then runs the two reference steps, which produce the reference's result or error exactly.
// =================================================================================================
bool filter_project_fused(Context& ctx, const Batch& rec, const std::vector<PlanColumn>& pcols, const Expr& pred,
                          const std::vector<chq_select_item>& fields, Batch* result) {
  const int64_t nrows = rec.nrows;
  if (ctx.opt_fuse == 0 || nrows < 2 || fields.empty()) return false;
  auto plain = [&](int ci) {   // fixed-width, no nulls
    const Column& c = rec.cols[ci];
    return c.type != T_BOOL && c.type != T_UTF8 && c.width > 0 && !(c.validity && c.null_count != 0);
  };
  struct Item { std::string name; bool nullable; int copy_col; int store_slot; DType type; };
  std::vector<Item> items;
  std::vector<TypedExpr> computed;
  Lowered lwp, lwq;
  try {
    TypedExpr tp = type_expr(pred, pcols, nrows, ctx.opt_enable_minus);
    if (!is_row_predicate(tp)) return false;
    lower_expr(tp, tp.root, pcols, lwp);
    if (!lwp.strs.empty()) return false;
    for (int ci : lwp.refs) if (!plain(ci)) return false;

    size_t unnamed_idx = 0;
    for (const chq_select_item& f : fields) {
      if (f.kind == CHQ_ITEM_WILDCARD) {
        for (size_t ci = 0; ci < rec.cols.size(); ++ci) {
          if (!plain((int)ci)) return false;
          items.push_back(Item{rec.cols[ci].name, rec.cols[ci].nullable, (int)ci, -1, rec.cols[ci].type});
        }
        continue;
      }
      if ((f.kind != CHQ_ITEM_UNNAMED_EXPR && f.kind != CHQ_ITEM_EXPR_WITH_ALIAS) || !f.expr) return false;
      const Expr& e = *(const Expr*)f.expr;
      TypedExpr te = type_expr(e, pcols, nrows, ctx.opt_enable_minus);
      if (te.pending_code) return false;
      const Node& root = te.at(te.root);
      if (root.len1) return false;   // a literal-built column: RecordBatch::try_new decides on the filtered length
      const std::string name = select_item_name(f, e, &unnamed_idx);
      if (root.kind == Node::COL) {
        if (!plain(root.col)) return false;
        items.push_back(Item{name, false, root.col, -1, rec.cols[root.col].type});
        continue;
      }
      if (root.type == T_BOOL || root.type == T_UTF8 || root.type == T_F16 || root.type == T_FIXED_OPAQUE) return false;
      if ((int)computed.size() >= MAX_PROJ) return false;
      lower_expr(te, te.root, pcols, lwq);
      Instr st{}; st.op = OP_STORE; st.src_idx = (uint16_t)computed.size(); st.src_kind = SRC_NONE;
      lwq.prog.push_back(st);
      if ((int)lwq.prog.size() > MAX_INSTR || !lwq.strs.empty()) return false;
      items.push_back(Item{name, false, -1, (int)computed.size(), root.type});
      computed.push_back(std::move(te));
    }
    for (int ci : lwq.refs) if (!plain(ci)) return false;
  } catch (const ChqError&) {
    return false;   // static errors are the two-step path's to report, in the reference's order
  }
  int n_copy = 0;
  for (const Item& it : items) n_copy += it.copy_col >= 0;
  if (n_copy > MAX_FUSED_COPY) return false;
  if (ctx.opt_fuse == 1 && nrows > (1 << 18)) {
    // (small batches are latency-bound: one launch and one synchronisation always beat two of each)
    // Worth it?  The single pass is instruction-bound (interpreter + compacting stores in one kernel) while the two
    // steps run near the HBM roofline, so it only pays when it moves clearly fewer bytes: the filter step copies the
    // WHOLE table, the single pass touches only what the predicate and the select items need.  Selectivity is not
    // known yet; 0.5 is assumed.  (Measured: 8-column table, 3 columns used: 3.2 ms vs 7.4 ms; config 3, 5 columns,
    // 4 used: 12.9 ms vs 12.4 ms.)
    double w_table = 0, w_pred = 0, w_proj = 0, w_out = 0;
    std::vector<char> in_pred(rec.cols.size(), 0), in_proj(rec.cols.size(), 0);
    for (const Column& c : rec.cols) w_table += c.width > 0 ? c.width : 16;
    for (int ci : lwp.refs) if (!in_pred[ci]) { in_pred[ci] = 1; w_pred += rec.cols[ci].width; }
    for (int ci : lwq.refs) if (!in_proj[ci]) { in_proj[ci] = 1; w_proj += rec.cols[ci].width; }
    for (const Item& it : items) {
      if (it.copy_col >= 0 && !in_proj[it.copy_col]) { in_proj[it.copy_col] = 1; w_proj += rec.cols[it.copy_col].width; }
      w_out += it.copy_col >= 0 ? rec.cols[it.copy_col].width : dtype_width(it.type);
    }
    const double two_steps = w_table + 0.5 * w_table + 0.5 * (w_proj + w_out);
    const double one_pass = w_pred + w_proj + 0.5 * w_out;
    if (two_steps < 2.0 * one_pass) return false;
  }

  const int tile_kind = (lwp.wide || lwq.wide || lwp.num_temps > 0 || lwq.num_temps > 0) ? 2
                        : (ctx.opt_tile_kind == 0 || ctx.opt_tile_kind == 1) ? (int)ctx.opt_tile_kind
                        : (nrows >= (1 << 18) ? 0 : 1);
  const int64_t tile_rows = kTileRows[tile_kind];
  const int64_t ntiles = (nrows + tile_rows - 1) / tile_rows;
  ensure_scratch(ctx, ntiles);

  ctx.stats = chq_call_stats{};
  ctx.stats.rows_in = nrows;
  Batch out;
  out.on_device = true; out.device_id = ctx.device;
  FusedParams p{};
  p.nrows = nrows; p.tile_begin = 0; p.tile_end = ntiles;
  bind_scratch(p, ctx);
  fill_refs(p.pred, lwp, rec, {});
  fill_refs(p.proj, lwq, rec, {});
  p.n_proj = (int32_t)computed.size();
  std::vector<char> read_once(rec.cols.size(), 0);
  for (int ci : lwp.refs) read_once[ci] = 1;
  for (int ci : lwq.refs) read_once[ci] = 1;
  int64_t out_width = 0;
  for (const Item& it : items) {
    Column o;
    o.name = it.name; o.nullable = it.nullable; o.type = it.type;
    if (it.copy_col >= 0) {
      const Column& c = rec.cols[it.copy_col];
      o.format = c.format; o.width = c.width;
      read_once[it.copy_col] = 1;
    } else {
      o.format = dtype_format(it.type); o.width = dtype_width(it.type);
    }
    auto vb = make_device_buffer((size_t)nrows * o.width + 16, ctx.device);
    o.values = (const uint8_t*)vb->ptr; o.owned.push_back(vb);
    if (it.copy_col >= 0) {
      OutCol& oc = p.copies[p.n_copy++];
      oc.in = rec.cols[it.copy_col].values0(); oc.out = vb->ptr; oc.width = (uint32_t)o.width;
    } else {
      ProjOut& po = p.outs[it.store_slot];
      po.values = vb->ptr; po.type = (uint8_t)it.type;
    }
    out_width += o.width;
    out.cols.push_back(std::move(o));
  }
  for (size_t ci = 0; ci < rec.cols.size(); ++ci) if (read_once[ci]) ctx.stats.bytes_read_alg += nrows * rec.cols[ci].width;

  clear_scratch(ctx, ntiles);
  kernel_span_begin(ctx);
  check_hip(launch_filter_project(p, tile_kind, (int)std::min<int64_t>(ntiles, grid_cap(ctx, tile_kind)), ctx.stream), "launch filter_project_kernel");
  kernel_span_end(ctx);
  const Scratch* hs = read_scratch(ctx);
  ctx.stats.kernel_ns += kernel_span_ns(ctx);
  if (hs->err != ERR_NONE) return false;
  const int64_t total = (int64_t)hs->total;
  for (Column& o : out.cols) o.length = total;
  out.nrows = total;
  ctx.stats.rows_out = total; ctx.stats.tiles = ntiles; ctx.stats.launches = 1;
  ctx.stats.bytes_written_alg = total * out_width;
  *result = std::move(out);
  return true;
}

// =================================================================================================
// project_record_host: project_record for a HOST batch with a host result (the materialize task's calling pattern,
// materialize_files_task.rs:110).  Only the columns the computed select items read are uploaded and only the computed
// columns come back; identifier and wildcard items -- columns handed through unchanged, often the wide Utf8 ones --
// are copied host to host and never cross PCIe.  False = outside its scope (an item fails typing, literal-only items,
// QualifiedWildcard ...): the general path decides, in the reference's order.
// =================================================================================================
bool project_record_host(Context& ctx, const std::vector<chq_select_item>& fields, const Batch& rec,
                         const chq_table_aliases* aliases, Batch* result) {
  if (rec.on_device || fields.empty()) return false;
  const int64_t nrows = rec.nrows;
  Batch host = rec;   // shallow: null counts resolved below
  for (Column& c : host.cols) if (c.validity && c.null_count < 0) c.null_count = count_nulls_host(c.validity, c.offset, c.length);
  const std::vector<PlanColumn> pcols = plan_columns(host, aliases);
  struct Item { int copy_col; int computed; std::string name; bool keep_schema_flag; };
  std::vector<Item> items;
  std::vector<TypedExpr> computed;
  try {
    size_t unnamed_idx = 0;
    for (const chq_select_item& f : fields) {
      if (f.kind == CHQ_ITEM_WILDCARD) {
        for (size_t ci = 0; ci < host.cols.size(); ++ci) items.push_back(Item{(int)ci, -1, host.cols[ci].name, true});
        continue;
      }
      if ((f.kind != CHQ_ITEM_UNNAMED_EXPR && f.kind != CHQ_ITEM_EXPR_WITH_ALIAS) || !f.expr) return false;
      const Expr& e = *(const Expr*)f.expr;
      TypedExpr te = type_expr(e, pcols, nrows, ctx.opt_enable_minus);
      if (te.pending_code) return false;
      const Node& root = te.at(te.root);
      if (root.len1) return false;
      const std::string name = select_item_name(f, e, &unnamed_idx);
      if (root.kind == Node::COL) { items.push_back(Item{root.col, -1, name, false}); continue; }
      items.push_back(Item{-1, (int)computed.size(), name, false});
      computed.push_back(std::move(te));
    }
  } catch (const ChqError&) {
    return false;
  }
  for (const Item& it : items)   // RecordBatch::try_new would refuse: let the general path say so
    if (it.copy_col >= 0 && it.keep_schema_flag && !host.cols[it.copy_col].nullable && host.cols[it.copy_col].null_count > 0) return false;

  ctx.stats = chq_call_stats{};
  ctx.stats.rows_in = nrows; ctx.stats.rows_out = nrows;
  std::vector<Column> results;
  if (!computed.empty()) {
    std::vector<char> needed(host.cols.size(), 0);
    for (const TypedExpr& te : computed) for (const Node& n : te.nodes) if (n.kind == Node::COL) needed[n.col] = 1;
    Batch dev;
    dev.nrows = nrows; dev.on_device = true; dev.device_id = ctx.device;
    for (size_t ci = 0; ci < host.cols.size(); ++ci) {
      if (needed[ci]) dev.cols.push_back(copy_column(ctx, host.cols[ci], Dir::H2D));
      else { Column ph = empty_like(host.cols[ci]); ph.length = nrows; dev.cols.push_back(std::move(ph)); }   // never dereferenced
    }
    std::vector<const TypedExpr*> ptrs;
    for (const TypedExpr& te : computed) ptrs.push_back(&te);
    std::vector<Column> dcols = evaluate_dense(ctx, dev, pcols, ptrs);
    for (Column& c : dcols) results.push_back(copy_column(ctx, c, Dir::D2H));
    check_hip(hipStreamSynchronize(ctx.stream), "hipStreamSynchronize");
  }
  Batch out;
  out.on_device = false; out.device_id = -1; out.nrows = nrows;
  for (const Item& it : items) {
    Column c;
    if (it.copy_col >= 0) {
      c = copy_column(ctx, host.cols[it.copy_col], Dir::H2H);
      c.nullable = it.keep_schema_flag ? host.cols[it.copy_col].nullable : c.null_count > 0;
      if (c.validity && c.null_count == 0) c.validity = nullptr;
    } else {
      c = std::move(results[(size_t)it.computed]);
      c.nullable = c.null_count > 0;
    }
    c.name = it.name;
    out.cols.push_back(std::move(c));
  }
  if (out.cols.empty()) return false;
  *result = std::move(out);
  return true;
}

// =================================================================================================
// describe_plan: the host half of a call (typing, coercion, constant folding, lowering) without a GPU
// =================================================================================================
std::string describe_plan(const ArrowSchema* schema, const chq_table_aliases* aliases, const Expr& expr, int64_t nrows,
                          bool enable_minus) {
  if (!schema || !schema->format || strcmp(schema->format, "+s") != 0)
    throw ChqError{CHQ_ERR_ARROW_INVALID_ARGUMENT, "record batch schema must be a struct"};
  std::vector<PlanColumn> cols;
  for (int64_t i = 0; i < schema->n_children; ++i) {
    const ArrowSchema* cs = schema->children[i];
    PlanColumn p;
    int width = 0;
    p.name = cs->name ? cs->name : "";
    parse_arrow_format(cs->format, &p.type, &width);
    p.format = cs->format ? cs->format : ""; p.width = width;
    p.has_nulls = (cs->flags & ARROW_FLAG_NULLABLE) != 0;
    p.alias_entry_present = aliases ? (int)i < aliases->n_columns : true;
    if (aliases && (int)i < aliases->n_columns)
      for (int k = 0; k < aliases->columns[i].n; ++k) p.aliases.push_back(aliases->columns[i].aliases[k]);
    cols.push_back(std::move(p));
  }
  TypedExpr te = type_expr(expr, cols, nrows, enable_minus);
  if (te.pending_code) throw ChqError{te.pending_code, te.pending_msg};
  const Node& root = te.at(te.root);
  static const char* kOps[] = {"LOAD", "ADD", "SUB", "MUL", "DIV", "REM", "EQ", "NE", "LT", "LE", "GT", "GE", "AND", "OR",
                               "CAST", "TOBOOL", "SPILL", "STRCMP", "STORE"};
  static const char* kSrc[] = {"-", "col", "const", "tmp", "btmp"};
  std::string out = std::string("result ") + dtype_name(root.type) + " scalar=" + (root.is_scalar ? "1" : "0") + " len1=" + (root.len1 ? "1" : "0") + "\n";
  if (root.len1) {
    Scalar v = fold_constant(te, te.root);
    char hex[40];
    snprintf(hex, sizeof hex, "%016llx", (unsigned long long)v.bits);
    out += std::string("value ") + (v.type == T_UTF8 ? "'" + v.str + "'" : std::string("0x") + hex) + "\n";
    return out;
  }
  if (root.kind == Node::COL) { out += "column " + std::to_string(root.col) + "\n"; return out; }
  Lowered lw;
  try {
    lower_expr(te, te.root, cols, lw);
  } catch (const ChqError& e) {
    if (e.code != CHQ_INTERNAL_PROGRAM_LIMIT) throw;
    // valid, but more than one device program: the engine evaluates sub-trees into temporary columns first (fit_to_device)
    out += "split " + e.msg + "\n";
    // the string functions of the tree, operands first: one line each, with the parts of a flattened `||` chain
    static const char* kStrFn[] = {"upper", "lower", "length", "octet_length", "substring", "trim", "ltrim", "rtrim", "concat"};
    std::function<void(int)> walk = [&](int ni) {
      const Node& n = te.at(ni);
      n.each_child(walk);
      if (n.kind != Node::STRFN) return;
      out += std::string("strfn ") + kStrFn[n.op];
      if (n.op == STRFN_CONCAT) out += " parts=" + std::to_string(n.parts.size());
      if (n.op == STRFN_SUBSTRING) out += " from=" + std::to_string(n.sub_p) + (n.sub_has_cnt ? " for=" + std::to_string(n.sub_cnt) : "");
      out += "\n";
    };
    walk(te.root);
    // the CASEs of the tree, operands first: WHENs, ELSE, result type, operands evaluated under a guard
    std::function<void(int)> cases = [&](int ni) {
      const Node& n = te.at(ni);
      n.each_child(cases);
      if (n.kind != Node::CASE) return;
      out += "case whens=" + std::to_string(n.op) + " else=" + (n.case_else ? "1" : "0") + " type=" + dtype_name(n.type) +
             " guarded=" + std::to_string(case_guarded_parts(te, ni, nullptr)) + "\n";
    };
    cases(te.root);
    // the explicit casts of the tree, operands first
    std::function<void(int)> casts = [&](int ni) {
      const Node& n = te.at(ni);
      n.each_child(casts);
      if (n.kind != Node::XCAST) return;
      out += std::string("cast ") + dtype_name(n.from) + " -> " + dtype_name(n.type) + (n.op ? " try" : "") + "\n";
    };
    casts(te.root);
    return out;
  }
  out += "program wide=" + std::to_string((int)lw.wide) + " num_temps=" + std::to_string(lw.num_temps) + " refs=";
  for (size_t i = 0; i < lw.refs.size(); ++i) out += (i ? "," : "") + std::to_string(lw.refs[i]);
  out += "\n";
  for (const Instr& in : lw.prog) {
    char line[160];
    snprintf(line, sizeof line, "  %-6s %-7s %s%s%s idx=%u%s imm=0x%llx\n", in.op < 19 ? kOps[in.op] : "?", dtype_name((DType)in.type),
             in.src_kind < 5 ? kSrc[in.src_kind] : "?", in.src_kind == SRC_COL ? ":" : "", in.src_kind == SRC_COL ? dtype_name((DType)in.src_type) : "",
             (unsigned)in.src_idx, (in.flags & IF_REV) ? " rev" : "", (unsigned long long)in.imm);
    out += line;
  }
  return out;
}

}  // namespace chq
