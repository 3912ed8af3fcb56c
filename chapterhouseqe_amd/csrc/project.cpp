// project.cpp -- dense evaluation of typed expressions, compute_value, the select-list reader and its three consumers
// (project_record, the fused filter + project pass, the host projection path) and describe_plan.  Reference map: project_record =
// RU/record_projection.rs:16-76, compute_value = RU/compute_value.rs:57-344 (RU = src/handlers/operator_handler/operators/record_utils).
#include "engine_internal.hpp"

#include <cstdio>
#include <cstring>

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

// one computed output of a launch: its position in the results; its counter slot, -1 when the expression cannot produce nulls
struct ProjItem { int out_index, null_slot; };

bool subtree_can_null(const TypedExpr& t, int ni, const std::vector<PlanColumn>& cols) {
  const Node& n = t.at(ni);
  if (n.kind == Node::COL) return cols[n.col].has_nulls;
  if (n.kind == Node::CONST) return n.cval.null;
  if (n.kind == Node::ISNULL) return false;   // IS [NOT] NULL is never null
  bool r = (n.kind == Node::TOBOOL && n.from == T_UTF8) ||   // a bad spelling is NULL
           (n.kind == Node::XCAST && n.op != 0 && cast_can_fail(n.from, n.type)) ||   // a failing TRY_CAST row too
           n.kind == Node::TPART || n.kind == Node::TTRUNC;   // a date outside the year range
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

// One output column of a select list, as project_record, the single-pass kernel and the host path all take it
struct SelectEntry {
  // a column of `*`, a column handed through, a literal-built length-1 value, a program to run
  enum Kind { WILDCARD, COLUMN, SCALAR, COMPUTED } kind = COMPUTED;
  std::string name;   // of the output column
  int col = -1;       // WILDCARD, COLUMN
  Scalar value;       // SCALAR
  TypedExpr typed;    // every kind but WILDCARD.  COMPUTED with pending_code set: a static error is due when the item is reached
  bool pending() const { return typed.pending_code != 0; }
};
struct SelectList {
  std::vector<SelectEntry> entries;
  ChqError stop{0, ""};           // code != 0: an item could not be read, `entries` holds what precedes it
  bool stop_after_earlier = true; // false: a broken item (null expr, unknown kind) is reported without evaluating anything
  bool stopped() const { return stop.code != 0; }
  // what the paths that only compute whole columns take: every item read, no length-1 value, no error pending
  bool whole_columns() const {
    for (const SelectEntry& en : entries) if (en.kind == SelectEntry::SCALAR || en.pending()) return false;
    return !stopped();
  }
};

// a typed expression as compute_value sorts it; a literal-only one is folded here (fold_constant may throw)
SelectEntry entry_of(TypedExpr te) {
  SelectEntry en;
  const Node& root = te.at(te.root);
  if (root.kind == Node::COL) { en.kind = SelectEntry::COLUMN; en.col = root.col; }
  else if (root.len1) { en.kind = SelectEntry::SCALAR; en.value = fold_constant(te, te.root); }
  en.typed = std::move(te);
  return en;
}

// THE reader of a select list (RU/record_projection.rs:16-76): kinds, `*`, typing, the three-way sort and the names, for a
// batch of `nrows` rows with the columns `pcols`.  Host work only, and nothing is thrown: the first item that cannot be read
// ends the list and its error is kept.
SelectList read_select_list(const std::vector<chq_select_item>& fields, const std::vector<PlanColumn>& pcols, int64_t nrows, bool enable_minus) {
  SelectList list;
  auto stop = [&](ChqError why, bool after_earlier) { list.stop = std::move(why); list.stop_after_earlier = after_earlier; };
  size_t unnamed_idx = 0;
  for (const chq_select_item& f : fields) {
    if (f.kind == CHQ_ITEM_WILDCARD) {   // :27-32
      for (size_t ci = 0; ci < pcols.size(); ++ci) list.entries.push_back(SelectEntry{SelectEntry::WILDCARD, pcols[ci].name, (int)ci, {}, {}});
      continue;
    }
    if (f.kind == CHQ_ITEM_QUALIFIED_WILDCARD) { stop({CHQ_ERR_PROJECT_NOT_IMPLEMENTED, "not implemented: SelectItem::QualifiedWildcard"}, true); break; }
    if (f.kind != CHQ_ITEM_UNNAMED_EXPR && f.kind != CHQ_ITEM_EXPR_WITH_ALIAS) { stop({CHQ_ERR_INVALID_HANDLE, "unknown select item kind"}, false); break; }
    if (!f.expr) { stop({CHQ_ERR_INVALID_HANDLE, "select item without expression"}, false); break; }
    const Expr& e = *(const Expr*)f.expr;
    SelectEntry en;
    try {
      TypedExpr te = type_expr(e, pcols, nrows, enable_minus);
      if (te.pending_code) en.typed = std::move(te); else en = entry_of(std::move(te));
    } catch (const ChqError& err) { stop(err, true); break; }
    en.name = select_item_name(f, e, &unnamed_idx);
    list.entries.push_back(std::move(en));
  }
  return list;
}

// the computed entries before `end`, in one evaluation
std::vector<Column> evaluate_entries(Context& ctx, const Batch& rec, const std::vector<PlanColumn>& pcols, const SelectList& list, size_t end) {
  std::vector<const TypedExpr*> ptrs;
  for (size_t i = 0; i < end; ++i) if (list.entries[i].kind == SelectEntry::COMPUTED) ptrs.push_back(&list.entries[i].typed);
  if (ptrs.empty()) return {};
  return evaluate_dense(ctx, rec, pcols, ptrs);
}

// The list cannot be produced: entry `at` has a static error pending, or (at = entries.size()) the list stopped there.  The
// reference evaluates the items one after the other, so what the caller gets is, strongest first:
//   1. the data-dependent error of any EARLIER computed item (the first failing one, as evaluate_dense finds it);
//   2. the data-dependent error of this item's own completed sub-trees (validate_roots; only when the batch has rows);
//   3. the static error of this item.
// A null `expr` and an unknown item kind are the exception: they are reported at once, without step 1 (QualifiedWildcard is
// an item of the reference's like any other and takes step 1).
[[noreturn]] void replay_stopped(Context& ctx, const Batch& rec, const std::vector<PlanColumn>& pcols, const SelectList& list, size_t at) {
  const bool pending = at < list.entries.size();
  if (pending || list.stop_after_earlier) (void)evaluate_entries(ctx, rec, pcols, list, at);   // 1
  if (pending) throw_pending(ctx, rec, pcols, list.entries[at].typed);                        // 2, 3
  throw list.stop;                                                                            // 3
}

// ---- evaluate_dense, step by step: which root may be a result, and the (still empty) column it becomes ---------------------
Column result_column(const Node& root, const std::vector<PlanColumn>& pcols, int64_t nrows) {
  Column o;
  o.type = root.type; o.format = dtype_format(root.type); o.width = dtype_width(root.type); o.length = nrows;
  // (a Utf8 result is a string function's: fitting turns it into a temporary column, which IS the result)
  // (.. or a CASE's, of any type)
  // (.. or a date_trunc's, of its operand's DataType)
  if ((root.kind == Node::CASE || root.kind == Node::TTRUNC) && root.type == T_FIXED_OPAQUE) { o.format = pcols[(size_t)root.fmt_col].format; o.width = pcols[(size_t)root.fmt_col].width; }
  // (.. or an explicit cast's to Utf8)
  if (root.kind != Node::CASE && root.kind != Node::TTRUNC && ((root.type == T_UTF8 && root.kind != Node::STRFN && root.kind != Node::XCAST) || root.type == T_FIXED_OPAQUE))
    throw ChqError{CHQ_ERR_NOT_SUPPORTED, std::string("expression result of type ") + dtype_name(root.type) + " is outside this build's scope"};
  return o;
}

// Too large for one program even alone: sub-trees become temporary columns first (fit_to_device), then the rest is
// evaluated like any other expression
Column evaluate_oversized(Context& ctx, const Batch& rec, const std::vector<PlanColumn>& pcols, const TypedExpr& te) {
  Batch work; std::vector<PlanColumn> wcols; TypedExpr fitted;
  fit_to_device(ctx, rec, pcols, te, work, wcols, fitted);
  if (fitted.at(fitted.root).kind == Node::COL) {   // a typed operation at the root: its temporary column is the result
    Column c = work.cols[(size_t)fitted.at(fitted.root).col];
    c.name.clear();
    return c;
  }
  return std::move(evaluate_dense(ctx, work, wcols, {&fitted})[0]);
}

struct Packed { Lowered lw; std::vector<ProjItem> items; };
// As many expressions from exprs[k] on as fit the program limits, for one launch; k moves past them
Packed pack_launch(const std::vector<const TypedExpr*>& exprs, const std::vector<PlanColumn>& pcols, size_t& k) {
  Packed pk;
  int null_slots = 0;
  const size_t k0 = k;
  for (; k < exprs.size() && (int)pk.items.size() < MAX_PROJ; ++k) {
    Lowered trial = pk.lw;
    try {
      lower_expr(*exprs[k], exprs[k]->root, pcols, trial);
      if ((int)trial.prog.size() + 1 > MAX_INSTR) throw ChqError{CHQ_ERR_NOT_SUPPORTED, "program too long"};
    } catch (const ChqError&) { if (k == k0) throw; break; }   // (throw: does not fit even alone)
    Instr st{}; st.op = OP_STORE; st.src_idx = (uint16_t)pk.items.size(); st.src_kind = SRC_NONE;
    trial.prog.push_back(st);
    pk.lw = std::move(trial);
    const bool can_null = subtree_can_null(*exprs[k], exprs[k]->root, pcols);
    if (can_null && null_slots >= 16) throw ChqError{CHQ_ERR_NOT_SUPPORTED, "too many nullable outputs in one projection"};
    pk.items.push_back(ProjItem{(int)k, can_null ? null_slots++ : -1});
  }
  return pk;
}

// One launch: the output buffers of pk's items, the kernel, the read-back of the error word and the null counts
void launch_packed(Context& ctx, const Batch& rec, const std::vector<PlanColumn>& pcols, const std::vector<const TypedExpr*>& exprs,
                   const Packed& pk, std::vector<Column>& results) {
  const int64_t nrows = rec.nrows;
  const std::vector<ProjItem>& items = pk.items;
  Scratch* ds = dev_scratch(ctx);   // (looked up here: a nested evaluation may have replaced the block)
  ProjectParams p{};
  p.nrows = nrows; p.err = &ds->err; p.n_proj = (int32_t)items.size();
  auto str_bufs = upload_strings(ctx, pk.lw);
  fill_refs(p.pb, pk.lw, rec, str_bufs);
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
  const int tile_kind = pick_tile_kind(ctx, pk.lw, nrows);
  launch_tiles(ctx, p, nrows, kTileRows[tile_kind], (int64_t)ctx.num_cus * (tile_kind == 0 ? 2 : 8), [&](bool partial, int grid, bool tail) {
    check_hip(launch_project(p, tile_kind, partial, grid, ctx.stream), tail ? "launch project_kernel (tail)" : "launch project_kernel");
  });
  const Scratch* hs = read_scratch(ctx);
  if (hs->err != ERR_NONE) {
    // Several expressions shared the launch and each numbers its nodes from zero, so the smallest (node, row) key may
    // belong to a later select item.  The reference evaluates the items one after the other: do the same to find
    // the error it would have reported.
    if (items.size() > 1) for (const ProjItem& it : items) (void)evaluate_dense(ctx, rec, pcols, {exprs[it.out_index]});   // throws at the first failing item
    throw_device_error(hs->err);
  }
  for (const ProjItem& it : items) {
    Column& o = results[it.out_index];
    if (it.null_slot >= 0) { o.null_count = (int64_t)hs->counters[it.null_slot]; if (o.null_count == 0) o.validity = nullptr; }
  }
}

}  // namespace

// Evaluate the expressions `exprs[k]` (typed trees) densely over `rec`; returns one column per expression.
std::vector<Column> evaluate_dense(Context& ctx, const Batch& rec, const std::vector<PlanColumn>& pcols, const std::vector<const TypedExpr*>& exprs) {
  std::vector<Column> results;
  for (const TypedExpr* te : exprs) results.push_back(result_column(te->at(te->root), pcols, rec.nrows));
  if (rec.nrows == 0) {
    for (Column& o : results) { give_empty_buffers(ctx, o); if (o.type == T_UTF8) o.data_bytes = 0; }
    check_hip(hipStreamSynchronize(ctx.stream), "sync");
    return results;
  }
  ensure_scratch(ctx, 1);
  for (size_t k = 0; k < exprs.size();) {
    if (!lowers_alone(*exprs[k], exprs[k]->root, pcols)) { results[k] = evaluate_oversized(ctx, rec, pcols, *exprs[k]); ++k; continue; }
    const Packed pk = pack_launch(exprs, pcols, k);
    launch_packed(ctx, rec, pcols, exprs, pk, results);
  }
  return results;
}

Column compute_value(Context& ctx, const Batch& rec, const std::vector<PlanColumn>& pcols, const Expr& expr, bool* is_scalar) {
  ctx.stats = chq_call_stats{};
  const SelectEntry en = entry_of(typed(ctx, rec, pcols, expr));
  if (is_scalar) *is_scalar = en.typed.at(en.typed.root).is_scalar;
  Column out;
  switch (en.kind) {
    case SelectEntry::COLUMN: out = clone_device_column(ctx, rec.cols[en.col]); check_hip(hipStreamSynchronize(ctx.stream), "sync"); break;
    case SelectEntry::SCALAR: out = scalar_column(ctx, en.value, ""); break;
    default: out = std::move(evaluate_dense(ctx, rec, pcols, {&en.typed})[0]); break;
  }
  out.nullable = out.null_count > 0;
  return out;
}

Batch project_record(Context& ctx, const std::vector<chq_select_item>& fields, const Batch& rec, const std::vector<PlanColumn>& pcols) {
  ctx.stats = chq_call_stats{};
  Batch out;
  out.on_device = true; out.device_id = ctx.device;
  const SelectList list = read_select_list(fields, pcols, rec.nrows, ctx.opt_enable_minus);
  size_t bad = 0;   // the first item that cannot be produced
  while (bad < list.entries.size() && !list.entries[bad].pending()) ++bad;
  if (bad < list.entries.size() || list.stopped()) replay_stopped(ctx, rec, pcols, list, bad);
  const size_t n_out = list.entries.size();   // (one entry per output column)
  auto kind = [&](size_t k) { return list.entries[k].kind; };
  for (const SelectEntry& en : list.entries) {   // the computed items stay empty until all are evaluated together
    Column col;
    if (en.kind == SelectEntry::SCALAR) col = scalar_column(ctx, en.value, en.name);
    else if (en.kind != SelectEntry::COMPUTED) col = clone_device_column(ctx, rec.cols[en.col]);
    out.cols.push_back(std::move(col));
  }
  std::vector<Column> cols = evaluate_entries(ctx, rec, pcols, list, n_out);
  for (size_t k = 0, next = 0; k < n_out; ++k) {
    if (kind(k) == SelectEntry::COMPUTED) out.cols[k] = std::move(cols[next++]);
    out.cols[k].name = list.entries[k].name;
  }
  // an identifier over a view keeps the view's bitmap with its null count unknown (imported as "may have nulls"): count the
  // window's nulls, so that its nullability is the reference's null_count > 0 below
  std::vector<size_t> counted;
  for (size_t k = 0; k < n_out; ++k) {
    Column& c = out.cols[k];
    if (kind(k) != SelectEntry::COLUMN) continue;
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
  for (size_t k = 0; k < out.cols.size(); ++k)
    if (kind(k) != SelectEntry::WILDCARD) out.cols[k].nullable = out.cols[k].null_count > 0;
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
namespace {
struct FusedPlan {
  struct Item { std::string name; bool nullable; int copy_col; int store_slot; DType type; };
  std::vector<Item> items;   // the output columns: a copy of an input column or a store slot of the select items' program
  Lowered lwp, lwq;          // the predicate; the computed select items, one OP_STORE each
  int n_computed = 0;
};

// Eligibility: a row predicate and a list of whole columns, over plain columns only, within the kernel's limits
bool plan_fused(Context& ctx, const Batch& rec, const std::vector<PlanColumn>& pcols, const Expr& pred, const std::vector<chq_select_item>& fields, FusedPlan& fp) {
  auto plain = [&](int ci) {   // fixed-width, no nulls
    const Column& c = rec.cols[ci];
    return c.type != T_BOOL && c.type != T_UTF8 && c.width > 0 && !(c.validity && c.null_count != 0);
  };
  int n_copy = 0;
  try {
    TypedExpr tp = type_expr(pred, pcols, rec.nrows, ctx.opt_enable_minus);
    if (!is_row_predicate(tp)) return false;
    lower_expr(tp, tp.root, pcols, fp.lwp);
    if (!fp.lwp.strs.empty()) return false;
    for (int ci : fp.lwp.refs) if (!plain(ci)) return false;
    // (static errors are the two steps' to report, in the reference's order; a literal-built column's length too: try_new's)
    const SelectList list = read_select_list(fields, pcols, rec.nrows, ctx.opt_enable_minus);
    if (!list.whole_columns()) return false;
    for (const SelectEntry& en : list.entries) {
      if (en.kind != SelectEntry::COMPUTED) {
        if (!plain(en.col) || ++n_copy > MAX_FUSED_COPY) return false;
        fp.items.push_back({en.name, en.kind == SelectEntry::WILDCARD && rec.cols[en.col].nullable, en.col, -1, rec.cols[en.col].type});
        continue;
      }
      const Node& root = en.typed.at(en.typed.root);
      if (root.type == T_BOOL || root.type == T_UTF8 || root.type == T_F16 || root.type == T_FIXED_OPAQUE) return false;
      if (fp.n_computed >= MAX_PROJ) return false;
      lower_expr(en.typed, en.typed.root, pcols, fp.lwq);
      Instr st{}; st.op = OP_STORE; st.src_idx = (uint16_t)fp.n_computed; st.src_kind = SRC_NONE;
      fp.lwq.prog.push_back(st);
      if ((int)fp.lwq.prog.size() > MAX_INSTR || !fp.lwq.strs.empty()) return false;
      fp.items.push_back({en.name, false, -1, fp.n_computed++, root.type});
    }
    for (int ci : fp.lwq.refs) if (!plain(ci)) return false;
  } catch (const ChqError&) {
    return false;   // the predicate does not type, or something does not lower: the two steps decide
  }
  return true;
}

// Worth it?  The single pass is instruction-bound (interpreter + compacting stores in one kernel) while the two
// steps run near the HBM roofline, so it only pays when it moves clearly fewer bytes: the filter step copies the
// WHOLE table, the single pass touches only what the predicate and the select items need.  Selectivity is not
// known yet; 0.5 is assumed.  (Measured: 8-column table, 3 columns used: 3.2 ms vs 7.4 ms; config 3, 5 columns,
// 4 used: 12.9 ms vs 12.4 ms.)
bool single_pass_pays(const Batch& rec, const FusedPlan& fp) {
  double w_table = 0, w_pred = 0, w_proj = 0, w_out = 0;
  std::vector<char> in_pred(rec.cols.size(), 0), in_proj(rec.cols.size(), 0);
  for (const Column& c : rec.cols) w_table += c.width > 0 ? c.width : 16;
  for (int ci : fp.lwp.refs) if (!in_pred[ci]) { in_pred[ci] = 1; w_pred += rec.cols[ci].width; }
  for (int ci : fp.lwq.refs) if (!in_proj[ci]) { in_proj[ci] = 1; w_proj += rec.cols[ci].width; }
  for (const FusedPlan::Item& it : fp.items) {
    if (it.copy_col >= 0 && !in_proj[it.copy_col]) { in_proj[it.copy_col] = 1; w_proj += rec.cols[it.copy_col].width; }
    w_out += it.copy_col >= 0 ? rec.cols[it.copy_col].width : dtype_width(it.type);
  }
  const double two_steps = w_table + 0.5 * w_table + 0.5 * (w_proj + w_out);
  const double one_pass = w_pred + w_proj + 0.5 * w_out;
  return two_steps >= 2.0 * one_pass;
}
}  // namespace

bool filter_project_fused(Context& ctx, const Batch& rec, const std::vector<PlanColumn>& pcols, const Expr& pred,
                          const std::vector<chq_select_item>& fields, Batch* result) {
  const int64_t nrows = rec.nrows;
  if (ctx.opt_fuse == 0 || nrows < 2 || fields.empty()) return false;
  FusedPlan fp;
  if (!plan_fused(ctx, rec, pcols, pred, fields, fp)) return false;
  // (small batches are latency-bound: one launch and one synchronisation always beat two of each)
  if (ctx.opt_fuse == 1 && nrows > (1 << 18) && !single_pass_pays(rec, fp)) return false;
  const Lowered &lwp = fp.lwp, &lwq = fp.lwq;

  // The launch.  (The tile kind is this kernel's own rule, not pick_tile_kind's.)
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
  p.n_proj = fp.n_computed;
  std::vector<char> read_once(rec.cols.size(), 0);
  for (int ci : lwp.refs) read_once[ci] = 1;
  for (int ci : lwq.refs) read_once[ci] = 1;
  int64_t out_width = 0;
  for (const FusedPlan::Item& it : fp.items) {
    const Column* c = it.copy_col >= 0 ? &rec.cols[it.copy_col] : nullptr;
    Column o;
    o.name = it.name; o.nullable = it.nullable; o.type = it.type;
    o.format = c ? c->format : dtype_format(it.type); o.width = c ? c->width : dtype_width(it.type);
    auto vb = make_device_buffer((size_t)nrows * o.width + 16, ctx.device);
    o.values = (const uint8_t*)vb->ptr; o.owned.push_back(vb);
    if (c) {
      read_once[it.copy_col] = 1;
      OutCol& oc = p.copies[p.n_copy++];
      oc.in = c->values0(); oc.out = vb->ptr; oc.width = (uint32_t)o.width;
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
  const SelectList list = read_select_list(fields, pcols, nrows, ctx.opt_enable_minus);
  if (!list.whole_columns()) return false;
  std::vector<const TypedExpr*> computed;
  for (const SelectEntry& en : list.entries) {
    if (en.kind == SelectEntry::COMPUTED) computed.push_back(&en.typed);
    // (a `*` column keeps its schema flag.)  RecordBatch::try_new would refuse: let the general path say so
    if (en.kind == SelectEntry::WILDCARD && !host.cols[en.col].nullable && host.cols[en.col].null_count > 0) return false;
  }

  ctx.stats = chq_call_stats{};
  ctx.stats.rows_in = nrows; ctx.stats.rows_out = nrows;
  std::vector<Column> results;
  if (!computed.empty()) {
    std::vector<char> needed(host.cols.size(), 0);
    for (const TypedExpr* te : computed) for (const Node& n : te->nodes) if (n.kind == Node::COL) needed[n.col] = 1;
    Batch dev;
    dev.nrows = nrows; dev.on_device = true; dev.device_id = ctx.device;
    for (size_t ci = 0; ci < host.cols.size(); ++ci) {
      if (needed[ci]) dev.cols.push_back(copy_column(ctx, host.cols[ci], Dir::H2D));
      else { Column ph = empty_like(host.cols[ci]); ph.length = nrows; dev.cols.push_back(std::move(ph)); }   // never dereferenced
    }
    std::vector<Column> dcols = evaluate_dense(ctx, dev, pcols, computed);
    for (Column& c : dcols) results.push_back(copy_column(ctx, c, Dir::D2H));
    check_hip(hipStreamSynchronize(ctx.stream), "hipStreamSynchronize");
  }
  Batch out;
  out.on_device = false; out.device_id = -1; out.nrows = nrows;
  size_t next_result = 0;
  for (const SelectEntry& en : list.entries) {
    Column c;
    if (en.kind != SelectEntry::COMPUTED) {
      c = copy_column(ctx, host.cols[en.col], Dir::H2H);
      c.nullable = en.kind == SelectEntry::WILDCARD ? host.cols[en.col].nullable : c.null_count > 0;
      if (c.validity && c.null_count == 0) c.validity = nullptr;
    } else {
      c = std::move(results[next_result++]);
      c.nullable = c.null_count > 0;
    }
    c.name = en.name;
    out.cols.push_back(std::move(c));
  }
  if (out.cols.empty()) return false;
  *result = std::move(out);
  return true;
}

// =================================================================================================
// describe_plan: the host half of a call (typing, coercion, constant folding, lowering) without a GPU
// =================================================================================================
// f(index, node) for every node of `kind` in the tree under `ni`, operands first; a node that several operators read (the
// operand of BETWEEN and IN) once, where it is first met
template <class F>
static void each_of_kind(const TypedExpr& te, int ni, Node::Kind kind, const F& f, std::vector<char>& seen) {
  if (seen[(size_t)ni]) return;
  seen[(size_t)ni] = 1;
  const Node& n = te.at(ni);
  n.each_child([&](int c) { each_of_kind(te, c, kind, f, seen); });
  if (n.kind == kind) f(ni, n);
}
template <class F>
static void each_of_kind(const TypedExpr& te, int ni, Node::Kind kind, const F& f) {
  std::vector<char> seen(te.nodes.size(), 0);
  each_of_kind(te, ni, kind, f, seen);
}

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
    each_of_kind(te, te.root, Node::STRFN, [&](int, const Node& n) {
      out += std::string("strfn ") + kStrFn[n.op];
      if (n.op == STRFN_CONCAT) out += " parts=" + std::to_string(n.parts.size());
      if (n.op == STRFN_SUBSTRING) out += " from=" + std::to_string(n.sub_p) + (n.sub_has_cnt ? " for=" + std::to_string(n.sub_cnt) : "");
      out += "\n";
    });
    // the CASEs of the tree, operands first: WHENs, ELSE, result type, operands evaluated under a guard
    each_of_kind(te, te.root, Node::CASE, [&](int ni, const Node& n) {
      out += "case whens=" + std::to_string(n.op) + " else=" + (n.case_else ? "1" : "0") + " type=" + dtype_name(n.type) +
             " guarded=" + std::to_string(case_guarded_parts(te, ni, nullptr)) + "\n";
    });
    // the explicit casts of the tree, operands first
    each_of_kind(te, te.root, Node::XCAST, [&](int, const Node& n) {
      out += std::string("cast ") + dtype_name(n.from) + " -> " + dtype_name(n.type) + (n.op ? " try" : "") + "\n";
    });
    // the temporal functions of the tree, operands first: the operand's kind; a date_trunc keeps its operand's Arrow format
    each_of_kind(te, te.root, Node::TPART, [&](int, const Node& n) {
      out += std::string("temporal part ") + kTemporalFieldNames[n.op] + " kind=" + std::to_string(n.tkind) + "\n";
    });
    each_of_kind(te, te.root, Node::TTRUNC, [&](int, const Node& n) {
      out += std::string("temporal trunc ") + kTemporalUnitNames[n.op] + " kind=" + std::to_string(n.tkind) + " format=" + cols[(size_t)n.fmt_col].format + "\n";
    });
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
