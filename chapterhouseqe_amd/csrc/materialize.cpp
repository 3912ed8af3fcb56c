// materialize.cpp -- expressions that do not fit one device program: sub-trees evaluated into temporary columns until the
// rest fits (fit_to_device), and the operators that are never device-program instructions and always become one -- LIKE,
// IS NULL, Decimal128 comparisons, Utf8 -> Boolean, the scalar string functions, CASE, CAST / TRY_CAST, EXTRACT / date_part and
// date_trunc.  filter.cpp and
// project.cpp (evaluate_dense) both come here.
#include "engine_internal.hpp"

namespace chq {

namespace {

// The reference has no size limits (one arrow kernel per AST node).  When lower_expr reports that a typed tree needs
// more instructions / columns / temporaries than a program holds, sub-trees are evaluated into temporary columns
// (appended to `work` / `wcols`, never part of any output) and replaced by column nodes, bottom-up and left to right
// -- i.e. in the reference's own evaluation order -- until the rest fits.  `strict` materialises EVERY inner node in
// that order (exactly the reference's strategy): used to find the first data-dependent error when a materialisation
// launch reports one, because a temporary may have been evaluated ahead of a smaller sub-tree to its left.
bool is_leaf_node(const Node& n) { return n.kind == Node::COL || n.kind == Node::CONST; }

// ---- the steps every temporary column shares --------------------------------------------------------------------------------
// The finished column `c` becomes a temporary of `work` / `wcols`, and the COL node that reads it replaces te.nodes[node].
void replace_by_column(Batch& work, std::vector<PlanColumn>& wcols, TypedExpr& te, int node, Column c) {
  c.name = "__chq_tmp_" + std::to_string(work.cols.size());
  PlanColumn pc;
  pc.name = c.name; pc.type = c.type; pc.has_nulls = c.live_validity() != nullptr; pc.alias_entry_present = true;
  pc.format = c.format; pc.width = c.width;
  Node repl{};
  repl.kind = Node::COL; repl.type = te.nodes[node].type; repl.is_scalar = false; repl.len1 = false;
  repl.col = (int)work.cols.size(); repl.ref_order = te.nodes[node].ref_order;
  work.cols.push_back(std::move(c));
  wcols.push_back(std::move(pc));
  te.nodes[node] = repl;
}

Column result_column(DType type, const std::string& format, int width, int64_t nrows) {
  Column c;
  c.type = type; c.format = format; c.width = width; c.length = nrows;
  return c;
}
// `c` as the result over a batch of no rows: no nulls, a values buffer of zeroes (a Utf8 column's offsets[0] == 0), no bytes
Column zero_row_result(Context& ctx, Column c) {
  auto vb = make_device_buffer(16, ctx.device);
  check_hip(hipMemsetAsync(vb->ptr, 0, 16, ctx.stream), "memset");
  c.values = (const uint8_t*)vb->ptr; c.owned.push_back(vb);
  if (c.type == T_UTF8) { auto db = make_device_buffer(16, ctx.device); c.data = (const uint8_t*)db->ptr; c.data_bytes = 0; c.owned.push_back(db); }
  check_hip(hipStreamSynchronize(ctx.stream), "sync");
  return c;
}

BufferPtr bitmap_buffer(Context& ctx, int64_t nrows) { return make_device_buffer(((size_t)((nrows + 63) / 64) + 1) * 8, ctx.device); }
// four 64-bit counters at zero: [0] is every kernel's null (or valid) count, the rest is the caller's
BufferPtr zeroed_counters(Context& ctx) {
  auto count = make_device_buffer(32, ctx.device);
  check_hip(hipMemsetAsync(count->ptr, 0, 32, ctx.stream), "memset");
  return count;
}
// the last step of every result: `valid` is kept, and the column nullable, only when a row came out null
void finish_nulls(Column& c, int64_t nulls, const BufferPtr& valid) {
  c.null_count = nulls; c.nullable = nulls != 0;
  if (nulls) { c.validity = (const uint8_t*)valid->ptr; c.owned.push_back(valid); }
}

void set_utf8_buffers(Column& c, const BufferPtr& offsets, const BufferPtr& data, int64_t bytes) {
  c.values = (const uint8_t*)offsets->ptr; c.data = (const uint8_t*)data->ptr; c.data_bytes = bytes;
  c.owned = {offsets, data};
}
// The Utf8 result `c` from its row lengths `d_len` (device, c.length of them): the offsets scan; ONE wait that brings the
// 64-bit byte total together with whatever `queue_reads()` asks for (the caller's null count, ..); a total that int32
// offsets cannot address refused as "the Utf8 result of <what> would hold ..."; then `gather(offsets, data)` queues the
// kernel that writes the bytes -- not when there are none -- and is waited for, so whatever it reads may go on return.
template <class Reads, class Gather>
void assemble_utf8(Context& ctx, Column& c, const void* d_len, const char* what, Reads&& queue_reads, Gather&& gather) {
  const int64_t nrows = c.length;
  OffsetsScanParams sp{};
  sp.len = (const uint32_t*)d_len; sp.n = nrows; sp.ntiles = (nrows + STRFN_SCAN_CHUNK - 1) / STRFN_SCAN_CHUNK;
  auto sums = make_device_buffer((size_t)(sp.ntiles + 1) * 8 + 16, ctx.device);
  auto offb = make_device_buffer((size_t)(nrows + 2) * 4, ctx.device);
  sp.tile_sums = (uint64_t*)sums->ptr; sp.out = (uint32_t*)offb->ptr; sp.write_total = 1;
  check_hip(launch_offsets_scan(sp, ctx.stream), "launch the offsets scan of the row lengths");
  queue_reads();
  u64 total = 0;
  check_hip(hipMemcpyAsync(&total, sp.tile_sums + sp.ntiles, 8, hipMemcpyDeviceToHost, ctx.stream), "read byte total");
  check_hip(hipStreamSynchronize(ctx.stream), "sync");
  if (total > (u64)INT32_MAX)
    throw ChqError{CHQ_ERR_ARROW_INVALID_ARGUMENT, std::string("the Utf8 result of ") + what + " would hold " + std::to_string(total) +
                                                   " bytes, more than int32 offsets can address"};
  auto db = make_device_buffer((size_t)total + 16, ctx.device);
  if (total > 0) {
    gather((const int32_t*)offb->ptr, (uint8_t*)db->ptr);
    check_hip(hipStreamSynchronize(ctx.stream), "sync");
  }
  set_utf8_buffers(c, offb, db, (int64_t)total);
}

// ---- a sub-tree that lowers into one program ---------------------------------------------------------------------------------
void materialize_node(Context& ctx, Batch& work, std::vector<PlanColumn>& wcols, TypedExpr& te, int node) {
  TypedExpr sub;
  sub.nodes = te.nodes; sub.root = node;
  std::vector<const TypedExpr*> one{&sub};
  const chq_call_stats keep = ctx.stats;
  std::vector<Column> cols = evaluate_dense(ctx, work, wcols, one);
  ctx.stats = keep;
  replace_by_column(work, wcols, te, node, std::move(cols[0]));
}

// Decimal128 comparisons, Utf8 -> Boolean casts, LIKE and IS [NOT] NULL are not device-program instructions (plan.hpp:
// Node): their own kernels (typed_ops.hip, like.hip) write a temporary Boolean column, which replaces the node like any
// other materialisation.  The scalar string functions (strfn.hip) do the same with a temporary Utf8 or Int32 column, CASE
// (case.hip) with a temporary column of its result type, CAST / TRY_CAST (cast.hip) with one of the target type.
bool is_typed_op(const TypedExpr& te, int node) {
  const Node& n = te.nodes[node];
  return (n.kind == Node::CMP && n.from == T_FIXED_OPAQUE) || (n.kind == Node::TOBOOL && n.from == T_UTF8) ||
         n.kind == Node::LIKE || n.kind == Node::ISNULL || n.kind == Node::STRFN || n.kind == Node::CASE || n.kind == Node::XCAST ||
         n.kind == Node::TPART || n.kind == Node::TTRUNC ||
         (n.kind == Node::CONST && n.cval.null);   // `'maybe' AND ..` folded to NULL, next to a column of a one-row batch
}
void fit_subtree(Context& ctx, Batch& work, std::vector<PlanColumn>& wcols, TypedExpr& te, int node, bool strict, bool is_root);

// ---- the Boolean operators (typed_ops.hip, like.hip) ------------------------------------------------
// The temporary Boolean column of node `n`: a NULL literal, IS [NOT] NULL, LIKE, a Decimal128 comparison or a Utf8 ->
// Boolean cast, whose operands are columns of `work`.
Column evaluate_bool_op(Context& ctx, const Batch& work, const TypedExpr& te, const Node& n) {
  if (n.kind == Node::CONST && n.type != T_BOOL)   // (nullif / CASE over literals can fold to one; only a Boolean one was ever met before)
    throw ChqError{CHQ_ERR_NOT_SUPPORTED, std::string("a NULL literal-built ") + dtype_name(n.type) + " value next to a column is outside this build's scope"};
  const int64_t nrows = work.nrows;
  Column c = result_column(T_BOOL, "b", 0, nrows);
  if (nrows == 0) return zero_row_result(ctx, std::move(c));
  const size_t words = (size_t)((nrows + 63) / 64) + 1;
  auto bits = bitmap_buffer(ctx, nrows), valid = bitmap_buffer(ctx, nrows);
  auto count = zeroed_counters(ctx);
  if (n.kind == Node::CONST) {   // every row null
    check_hip(hipMemsetAsync(bits->ptr, 0, words * 8, ctx.stream), "memset");
    check_hip(hipMemsetAsync(valid->ptr, 0, words * 8, ctx.stream), "memset");
  } else if (n.kind == Node::ISNULL) {
    const Column& a = work.cols[(size_t)te.nodes[n.l].col];
    IsNullParams p{};
    p.validity = a.live_validity(); p.validity_offset = a.offset;
    p.nrows = nrows; p.negated = n.op; p.out_bits = (u64*)bits->ptr;
    check_hip(launch_is_null(p, ctx.stream), "launch is_null_kernel");
  } else if (n.kind == Node::LIKE) {
    const Column& a = work.cols[(size_t)te.nodes[n.l].col];
    LikeParams p{};
    p.offsets = (const int32_t*)a.values0(); p.data = a.data;
    p.validity = a.live_validity(); p.validity_offset = a.offset;
    p.nrows = nrows; p.negated = n.op; p.pat = *n.like;
    p.out_bits = (u64*)bits->ptr; p.out_validity = (u64*)valid->ptr; p.null_count = (u64*)count->ptr;
    check_hip(launch_like(p, ctx.stream), "launch like_kernel");
  } else if (n.kind == Node::CMP) {
    const Column& a = work.cols[(size_t)te.nodes[n.l].col];
    const Column& b = work.cols[(size_t)te.nodes[n.r].col];
    Cmp128Params p{};
    p.a = a.values0(); p.b = b.values0();
    p.a_validity = a.live_validity(); p.a_validity_offset = a.offset;
    p.b_validity = b.live_validity(); p.b_validity_offset = b.offset;
    p.nrows = nrows; p.op = n.op;
    p.out_bits = (u64*)bits->ptr; p.out_validity = (u64*)valid->ptr; p.null_count = (u64*)count->ptr;
    check_hip(launch_cmp128(p, ctx.stream), "launch cmp128_kernel");
  } else {
    const Column& a = work.cols[(size_t)te.nodes[n.l].col];
    Utf8ToBoolParams p{};
    p.offsets = (const int32_t*)a.values0(); p.data = a.data;
    p.validity = a.live_validity(); p.validity_offset = a.offset;
    p.nrows = nrows;
    p.out_bits = (u64*)bits->ptr; p.out_validity = (u64*)valid->ptr; p.null_count = (u64*)count->ptr;
    check_hip(launch_utf8_to_bool(p, ctx.stream), "launch utf8_to_bool_kernel");
  }
  u64 nulls = 0;
  check_hip(hipMemcpyAsync(&nulls, count->ptr, 8, hipMemcpyDeviceToHost, ctx.stream), "read null count");
  check_hip(hipStreamSynchronize(ctx.stream), "sync");
  c.values = (const uint8_t*)bits->ptr; c.owned = {bits};
  finish_nulls(c, n.kind == Node::CONST ? nrows : (int64_t)nulls, valid);
  return c;
}

// ---- the scalar string functions (strfn.hip) ------------------------------------------------------
StrPart column_part(const Column& c) {
  StrPart q{};
  q.offsets = (const int32_t*)c.values0(); q.data = c.data;
  q.validity = c.live_validity(); q.validity_offset = c.offset;
  return q;
}
// The temporary column of STRFN node `n`, whose operands are columns of `work` (or, for `||`, Utf8 literals).
Column evaluate_strfn(Context& ctx, const Batch& work, const TypedExpr& te, const Node& n) {
  const int64_t nrows = work.nrows;
  Column c = result_column(n.type, n.type == T_UTF8 ? "u" : "i", n.type == T_UTF8 ? 0 : 4, nrows);
  if (nrows == 0) return zero_row_result(ctx, std::move(c));
  auto valid = bitmap_buffer(ctx, nrows);
  auto count = zeroed_counters(ctx);   // [0] null count (or valid count)
  u64 h_count = 0;
  auto read_count = [&] { check_hip(hipMemcpyAsync(&h_count, count->ptr, 8, hipMemcpyDeviceToHost, ctx.stream), "read null count"); };
  if (n.op == STRFN_UPPER || n.op == STRFN_LOWER) {
    // the length is preserved: the input's offsets rebased to 0, a flat map over its byte range, its validity re-aligned
    const Column& sc = work.cols[(size_t)te.nodes[n.l].col];
    const int32_t* offs = (const int32_t*)sc.values0();
    const bool may_null = sc.live_validity() != nullptr;
    if (may_null) {
      IsNullParams ip{};
      ip.validity = sc.validity; ip.validity_offset = sc.offset; ip.nrows = nrows; ip.negated = 1; ip.out_bits = (u64*)valid->ptr;
      check_hip(launch_is_null(ip, ctx.stream), "launch is_null_kernel");
      check_hip(launch_count_bits(sc.validity, sc.offset, nrows, (u64*)count->ptr, ctx.stream), "launch count_bits_kernel");
    }
    int32_t ends[2] = {0, 0};
    check_hip(hipMemcpyAsync(&ends[0], offs, 4, hipMemcpyDeviceToHost, ctx.stream), "read first offset");
    check_hip(hipMemcpyAsync(&ends[1], offs + nrows, 4, hipMemcpyDeviceToHost, ctx.stream), "read last offset");
    read_count();   // (rows valid)
    check_hip(hipStreamSynchronize(ctx.stream), "sync");
    const int64_t bytes = (int64_t)ends[1] - ends[0];
    auto offb = make_device_buffer((size_t)(nrows + 2) * 4, ctx.device), db = make_device_buffer((size_t)bytes + 16, ctx.device);
    StrRebaseParams rp{offs, (int32_t*)offb->ptr, nrows + 1};
    check_hip(launch_strfn_rebase(rp, ctx.stream), "launch strfn_rebase_kernel");
    if (bytes > 0) {
      StrByteMapParams bp{sc.data + ends[0], (uint8_t*)db->ptr, bytes, n.op == STRFN_UPPER ? 1 : 0, 0};
      check_hip(launch_strfn_bytemap(bp, ctx.stream), "launch strfn_bytemap_kernel");
    }
    check_hip(hipStreamSynchronize(ctx.stream), "sync");
    set_utf8_buffers(c, offb, db, bytes);
    finish_nulls(c, may_null ? nrows - (int64_t)h_count : 0, valid);
    return c;
  }
  StrRowsParams rp{};
  std::vector<BufferPtr> lits;   // (with the windows: let go on return, after the last wait)
  if (n.op == STRFN_CONCAT) {
    for (int ci : n.parts) {
      const Node& pn = te.nodes[(size_t)ci];
      StrPart& q = rp.part[rp.n_parts++];
      if (pn.kind == Node::COL) { q = column_part(work.cols[(size_t)pn.col]); continue; }
      lits.push_back(upload_literal(ctx, pn.cval.str));
      q.data = (const uint8_t*)lits.back()->ptr; q.lit_len = (int32_t)pn.cval.str.size();
    }
  } else {
    rp.part[0] = column_part(work.cols[(size_t)te.nodes[n.l].col]);
    rp.n_parts = 1;
  }
  rp.fn = n.op; rp.p = n.sub_p; rp.cnt = n.sub_cnt; rp.has_cnt = n.sub_has_cnt ? 1 : 0; rp.nrows = nrows;
  auto i32 = make_device_buffer((size_t)nrows * 4 + 16, ctx.device);   // the Int32 result, or the row lengths of the Utf8 one
  rp.out_i32 = (int32_t*)i32->ptr; rp.out_validity = (u64*)valid->ptr; rp.null_count = (u64*)count->ptr;
  const bool windowed = n.op != STRFN_CONCAT && n.type == T_UTF8;   // SUBSTRING / TRIM: one source range per row
  BufferPtr start;
  if (windowed) { start = make_device_buffer((size_t)nrows * 4 + 16, ctx.device); rp.out_start = (int32_t*)start->ptr; }
  check_hip(launch_strfn_rows(rp, ctx.stream), "launch strfn_rows_kernel");
  if (n.type == T_I32) {
    read_count();
    check_hip(hipStreamSynchronize(ctx.stream), "sync");
    c.values = (const uint8_t*)i32->ptr; c.owned = {i32};
  } else {
    assemble_utf8(ctx, c, i32->ptr, "a string function", read_count, [&](const int32_t* offsets, uint8_t* data) {
      StrGatherParams gp{};
      for (int k = 0; k < rp.n_parts; ++k) gp.part[k] = rp.part[k];
      gp.n_parts = rp.n_parts; gp.nrows = nrows; gp.start = windowed ? (const int32_t*)start->ptr : nullptr;
      gp.out_offsets = offsets; gp.out_data = data;
      check_hip(launch_strfn_gather(gp, ctx.stream), "launch strfn_gather_kernel");
    });
  }
  finish_nulls(c, (int64_t)h_count, valid);
  return c;
}

// ---- CASE, COALESCE, NULLIF (case.hip) ------------------------------------------------------------
// A copy of the sub-tree at `node`, appended to te.nodes, that reads VIEWS of its columns: the same values, a validity that is
// the column's AND `guard` (words aligned to bit 0).  kernels.hip raises data-dependent errors on valid slots only, so the
// copy reports nothing on rows outside the guard and is null there.  The views are appended to `work` / `wcols`.
int guarded_copy(Context& ctx, Batch& work, std::vector<PlanColumn>& wcols, TypedExpr& te, int node, const u64* guard,
                 std::vector<std::pair<int, int>>& views) {
  Node n = te.nodes[(size_t)node];
  if (n.kind == Node::COL) {
    int vi = -1;
    for (const auto& v : views) if (v.first == n.col) vi = v.second;
    if (vi < 0) {
      const int64_t nrows = work.nrows;
      Column v = work.cols[(size_t)n.col];
      PlanColumn pc = wcols[(size_t)n.col];
      auto vb = bitmap_buffer(ctx, nrows);
      CaseAndParams ap{v.live_validity(), v.offset, guard, nrows, (u64*)vb->ptr};
      check_hip(launch_case_and(ap, ctx.stream), "launch case_and_kernel");
      if (v.type == T_BOOL) {   // the values of a Boolean column are read from the same bit offset: re-aligned too
        auto bb = bitmap_buffer(ctx, nrows);
        CaseAndParams bp{v.values, v.offset, nullptr, nrows, (u64*)bb->ptr};
        check_hip(launch_case_and(bp, ctx.stream), "launch case_and_kernel");
        v.values = (const uint8_t*)bb->ptr; v.owned.push_back(bb);
      } else {
        v.values = (const uint8_t*)v.values0();
      }
      v.offset = 0; v.validity = (const uint8_t*)vb->ptr; v.null_count = -1; v.owned.push_back(vb);
      v.name = "__chq_view_" + std::to_string(work.cols.size());
      pc.name = v.name; pc.has_nulls = true;
      vi = (int)work.cols.size();
      work.cols.push_back(std::move(v));
      wcols.push_back(std::move(pc));
      views.emplace_back(n.col, vi);
    }
    n.col = vi;
  } else {
    if (n.l >= 0) n.l = guarded_copy(ctx, work, wcols, te, n.l, guard, views);
    if (n.r >= 0) n.r = guarded_copy(ctx, work, wcols, te, n.r, guard, views);
    for (int& c : n.parts) c = guarded_copy(ctx, work, wcols, te, c, guard, views);
  }
  te.nodes.push_back(std::move(n));
  return (int)te.nodes.size() - 1;
}

// The temporary column of CASE node `node`.  Operands are evaluated in the order c1..cn, r1..rn, else; one that can fail on
// data (case_guarded_parts) is evaluated under its guard -- a result under its take mask, a condition under what remained
// after the WHENs before it, so the masks are then built WHEN by WHEN -- and everything else unguarded, all masks in one launch.
Column evaluate_case(Context& ctx, Batch& work, std::vector<PlanColumn>& wcols, TypedExpr& te, int node, bool strict) {
  const int64_t nrows = work.nrows;
  const Node head = te.nodes[(size_t)node];
  const int nw = head.op;
  const PlanColumn* like = head.type == T_FIXED_OPAQUE ? &wcols[(size_t)head.fmt_col] : nullptr;
  Column c = result_column(head.type, like ? like->format : dtype_format(head.type), like ? like->width : dtype_width(head.type), nrows);
  if (nrows == 0) return zero_row_result(ctx, std::move(c));
  const int64_t words = (nrows + 63) / 64;
  auto masks = make_device_buffer((size_t)(nw + 1) * (size_t)words * 8 + 16, ctx.device);   // (with the literals: let go on return)
  u64* const d_masks = (u64*)masks->ptr;
  std::vector<char> guard;
  case_guarded_parts(te, node, &guard);
  // an operand as a column or a literal: fitted, evaluated (under `g` when it is guarded) and replaced
  auto operand = [&](size_t j, const u64* g) {
    int q = te.nodes[(size_t)node].parts[j];
    if (te.nodes[(size_t)q].kind == Node::CONST) return;
    if (guard[j]) {
      std::vector<std::pair<int, int>> views;
      q = guarded_copy(ctx, work, wcols, te, q, g, views);
      te.nodes[(size_t)node].parts[j] = q;
    }
    fit_subtree(ctx, work, wcols, te, q, strict, false);
    if (te.nodes[(size_t)q].kind != Node::COL) materialize_node(ctx, work, wcols, te, q);
  };
  int done = 0;   // WHENs whose take masks are written
  auto masks_through = [&](int k1) {
    if (k1 <= done) return;
    CaseMasksParams mp{};
    mp.first = done; mp.n = k1 - done; mp.n_total = nw; mp.nrows = nrows; mp.words = words; mp.masks = d_masks;
    for (int k = done; k < k1; ++k) {
      const Node& cn = te.nodes[(size_t)te.nodes[(size_t)node].parts[(size_t)k]];
      CaseCond& cc = mp.cond[k - done];
      if (cn.kind == Node::CONST) { cc.kind = cn.cval.null ? CASE_NULL : CASE_CONST; cc.const_val = (int32_t)(cn.cval.bits & 1); continue; }
      const Column& col = work.cols[(size_t)cn.col];
      cc.kind = CASE_COLUMN; cc.values = col.values; cc.validity = col.live_validity(); cc.offset = col.offset;
    }
    check_hip(launch_case_masks(mp, ctx.stream), "launch case_masks_kernel");
    done = k1;
  };
  for (int k = 0; k < nw; ++k) {
    if (guard[(size_t)k]) masks_through(k);   // (its guard: what remained after the WHENs before it)
    operand((size_t)k, d_masks + (size_t)nw * (size_t)words);
  }
  masks_through(nw);
  for (size_t j = (size_t)nw; j < head.parts.size(); ++j) operand(j, d_masks + (j - (size_t)nw) * (size_t)words);

  CaseSelectParams sp{};
  std::vector<BufferPtr> lits;
  sp.n_when = nw; sp.width = c.width; sp.nrows = nrows; sp.words = words; sp.masks = d_masks;
  for (int k = 0; k <= nw; ++k) {
    CaseBranch& b = sp.br[k];
    if (k == nw && !head.case_else) { b.kind = CASE_NULL; continue; }
    const Node& rn = te.nodes[(size_t)te.nodes[(size_t)node].parts[(size_t)(nw + k)]];
    if (rn.kind == Node::CONST) {
      if (rn.cval.null) { b.kind = CASE_NULL; continue; }
      b.kind = CASE_CONST; b.const_lo = rn.cval.bits;
      if (head.type == T_UTF8) {
        lits.push_back(upload_literal(ctx, rn.cval.str));
        b.data = (const uint8_t*)lits.back()->ptr; b.lit_len = (int32_t)rn.cval.str.size();
      }
      continue;
    }
    const Column& col = work.cols[(size_t)rn.col];
    b.kind = CASE_COLUMN;
    b.values = head.type == T_BOOL ? col.values : (const uint8_t*)col.values0();
    b.data = col.data; b.validity = col.live_validity(); b.offset = col.offset;
  }
  auto valid = bitmap_buffer(ctx, nrows);
  auto count = zeroed_counters(ctx);
  sp.out_validity = (u64*)valid->ptr; sp.null_count = (u64*)count->ptr;
  u64 h_count = 0;
  auto read_count = [&] { check_hip(hipMemcpyAsync(&h_count, count->ptr, 8, hipMemcpyDeviceToHost, ctx.stream), "read null count"); };
  if (head.type == T_UTF8) {
    auto len = make_device_buffer((size_t)nrows * 4 + 16, ctx.device);
    sp.out_len = (int32_t*)len->ptr;
    check_hip(launch_case_rows(sp, ctx.stream), "launch case_rows_kernel");
    assemble_utf8(ctx, c, len->ptr, "CASE", read_count, [&](const int32_t* offsets, uint8_t* data) {
      sp.out_offsets = offsets; sp.out_data = data;
      check_hip(launch_case_gather(sp, ctx.stream), "launch case_gather_kernel");
    });
  } else {
    const size_t vbytes = head.type == T_BOOL ? (size_t)(words + 1) * 8 : (size_t)nrows * (size_t)c.width + 16;
    auto vb = make_device_buffer(vbytes, ctx.device);
    sp.out_values = vb->ptr;
    if (head.type == T_BOOL) check_hip(launch_case_select_bool(sp, ctx.stream), "launch case_select_bool_kernel");
    else check_hip(launch_case_select_fixed(sp, ctx.stream), "launch case_select_fixed_kernel");
    read_count();
    check_hip(hipStreamSynchronize(ctx.stream), "sync");
    c.values = (const uint8_t*)vb->ptr; c.owned = {vb};
  }
  finish_nulls(c, (int64_t)h_count, valid);
  return c;
}

// ---- CAST, TRY_CAST (cast.hip) ---------------------------------------------------------------------
// The temporary column of XCAST node `n`, whose operand is a column of `work`.  A CAST fails with CHQ_ERR_ARROW_CAST when a
// VALID row cannot be converted; under TRY_CAST such rows are null.
Column evaluate_cast(Context& ctx, const Batch& work, const TypedExpr& te, const Node& n) {
  const int64_t nrows = work.nrows;
  const Column& sc = work.cols[(size_t)te.nodes[n.l].col];
  const DType from = n.from, to = n.type;
  const bool try_cast = n.op != 0;
  Column c = result_column(to, dtype_format(to), dtype_width(to), nrows);
  if (nrows == 0) return zero_row_result(ctx, std::move(c));
  const size_t words = (size_t)((nrows + 63) / 64) + 1;
  const void* in_validity = sc.live_validity();
  auto valid = bitmap_buffer(ctx, nrows);
  // [0] rows valid in the output, [1] the failure flag (low 32 bits), [2] rows valid in the input (Utf8 -> Boolean)
  auto count = zeroed_counters(ctx);
  u64* const d_count = (u64*)count->ptr;
  u64 h_count[3] = {0, 0, 0};
  auto read_counts = [&] {
    check_hip(launch_count_bits((const uint8_t*)valid->ptr, 0, nrows, d_count, ctx.stream), "launch count_bits_kernel");
    check_hip(hipMemcpyAsync(h_count, d_count, 24, hipMemcpyDeviceToHost, ctx.stream), "read valid count and failure flag");
  };
  bool failed = false;
  if (to == T_UTF8) {   // integer / Boolean -> Utf8: lengths, offsets, bytes
    CastPrintParams p{};
    p.values = from == T_BOOL ? (const void*)sc.values : sc.values0(); p.values_offset = from == T_BOOL ? sc.offset : 0;
    p.validity = in_validity; p.validity_offset = sc.offset; p.nrows = nrows; p.from = from;
    auto len = make_device_buffer((size_t)nrows * 4 + 16, ctx.device);   // (let go on return)
    p.out_len = (uint32_t*)len->ptr; p.out_validity = (u64*)valid->ptr;
    check_hip(launch_cast_len(p, ctx.stream), "launch cast_len_kernel");
    assemble_utf8(ctx, c, len->ptr, "a cast", read_counts, [&](const int32_t* offsets, uint8_t* data) {
      p.out_offsets = offsets; p.out_data = data;
      check_hip(launch_cast_write(p, ctx.stream), "launch cast_write_kernel");
    });
  } else if (from == T_UTF8 && to == T_BOOL) {
    // the kernel of the cast under AND / OR: a spelling it does not know comes out null.  CAST: such a row on a valid input
    // row is the failure, i.e. the output holds fewer valid rows than the input
    auto bits = make_device_buffer(words * 8, ctx.device);
    Utf8ToBoolParams p{};
    p.offsets = (const int32_t*)sc.values0(); p.data = sc.data;
    p.validity = in_validity; p.validity_offset = sc.offset; p.nrows = nrows;
    p.out_bits = (u64*)bits->ptr; p.out_validity = (u64*)valid->ptr; p.null_count = d_count + 3;   // (not read)
    check_hip(launch_utf8_to_bool(p, ctx.stream), "launch utf8_to_bool_kernel");
    if (in_validity) check_hip(launch_count_bits(sc.validity, sc.offset, nrows, d_count + 2, ctx.stream), "launch count_bits_kernel");
    read_counts();
    check_hip(hipStreamSynchronize(ctx.stream), "sync");
    failed = !try_cast && h_count[0] != (in_validity ? h_count[2] : (u64)nrows);
    c.values = (const uint8_t*)bits->ptr; c.owned = {bits};
  } else {
    const size_t vbytes = to == T_BOOL ? words * 8 : (size_t)nrows * (size_t)c.width + 16;
    auto vb = make_device_buffer(vbytes, ctx.device);
    if (from == T_UTF8) {
      CastParseParams p{};
      p.offsets = (const int32_t*)sc.values0(); p.data = sc.data;
      p.validity = in_validity; p.validity_offset = sc.offset; p.nrows = nrows; p.to = to; p.try_cast = try_cast ? 1 : 0;
      p.out_values = vb->ptr; p.out_validity = (u64*)valid->ptr; p.fail = (uint32_t*)(d_count + 1);
      check_hip(launch_cast_parse(p, ctx.stream), "launch cast_parse_kernel");
    } else {
      CastFixedParams p{};
      p.values = from == T_BOOL ? (const void*)sc.values : sc.values0(); p.values_offset = from == T_BOOL ? sc.offset : 0;
      p.validity = in_validity; p.validity_offset = sc.offset; p.nrows = nrows;
      p.from = from; p.to = to; p.try_cast = try_cast ? 1 : 0;
      p.out_values = vb->ptr; p.out_validity = (u64*)valid->ptr; p.fail = (uint32_t*)(d_count + 1);
      check_hip(launch_cast_fixed(p, ctx.stream), "launch cast_fixed_kernel");
    }
    read_counts();
    check_hip(hipStreamSynchronize(ctx.stream), "sync");
    failed = (uint32_t)h_count[1] != 0;
    c.values = (const uint8_t*)vb->ptr; c.owned = {vb};
  }
  if (failed)
    throw ChqError{CHQ_ERR_ARROW_CAST, std::string("Cast error: a ") + dtype_name(from) + " value cannot be cast to " + dtype_name(to)};
  finish_nulls(c, nrows - (int64_t)h_count[0], valid);
  return c;
}

// ---- EXTRACT / date_part, date_trunc (temporal.hip) ------------------------------------------------
// The temporary column of TPART / TTRUNC node `n`, whose operand is a column of `work`: an Int32 column, or one of the operand's
// own DataType.  No row fails; the rows the null rule of temporal_device.h makes null are counted by the kernel.
Column evaluate_temporal(Context& ctx, const Batch& work, const TypedExpr& te, const Node& n) {
  const int64_t nrows = work.nrows;
  const Column& sc = work.cols[(size_t)te.nodes[n.l].col];
  const bool part = n.kind == Node::TPART;
  Column c = part ? result_column(T_I32, "i", 4, nrows) : result_column(T_FIXED_OPAQUE, sc.format, sc.width, nrows);
  if (nrows == 0) return zero_row_result(ctx, std::move(c));
  auto valid = bitmap_buffer(ctx, nrows);
  auto count = zeroed_counters(ctx);
  auto vb = make_device_buffer((size_t)nrows * (size_t)c.width + 16, ctx.device);
  TemporalParams p{};
  p.values = sc.values; p.values_offset = sc.offset; p.validity = sc.live_validity(); p.validity_offset = sc.offset;
  p.nrows = nrows; p.kind = n.tkind; p.op = n.op;
  p.out_values = vb->ptr; p.out_validity = (u64*)valid->ptr; p.null_count = (u64*)count->ptr;
  kernel_span_begin(ctx);
  check_hip(part ? launch_temporal_part(p, ctx.stream) : launch_temporal_trunc(p, ctx.stream), part ? "launch temporal_part_kernel" : "launch temporal_trunc_kernel");
  kernel_span_end(ctx);
  u64 nulls = 0;
  check_hip(hipMemcpyAsync(&nulls, count->ptr, 8, hipMemcpyDeviceToHost, ctx.stream), "read null count");
  check_hip(hipStreamSynchronize(ctx.stream), "sync");
  // (a call's counters: the values read and written once, the validity words in and out)
  ++ctx.typed_stats.launches;
  ctx.typed_stats.kernel_ns += kernel_span_ns(ctx);   // (0 unless `time_kernels` is set)
  ctx.typed_stats.bytes_read_alg += nrows * sc.width + (p.validity ? (nrows + 7) / 8 : 0);
  ctx.typed_stats.bytes_written_alg += nrows * c.width + (nrows + 7) / 8;
  c.values = (const uint8_t*)vb->ptr; c.owned = {vb};
  finish_nulls(c, (int64_t)nulls, valid);
  return c;
}

// A typed operation becomes a temporary column in three steps: its operands as columns, its own kernels, the replacement.
void materialize_typed_op(Context& ctx, Batch& work, std::vector<PlanColumn>& wcols, TypedExpr& te, int node, bool strict) {
  const Node::Kind kind = te.nodes[node].kind;
  if (kind != Node::CASE) {   // (CASE brings its own, some of them under guards: evaluate_case)
    // the operands as columns: a computed one (a literal-only one was folded at typing) is evaluated first, with its
    // data-dependent errors, in the order `strict` asks for.  Until the string functions only IS NULL and LIKE had operands
    // that were not columns; a Utf8 -> Boolean cast takes this route too now, for `upper(s) AND b` (its operand was always a
    // column before, which this leaves alone).  A literal part of `||` -- and of `||` only -- stays a literal.
    const bool is_concat = kind == Node::STRFN && te.nodes[node].op == STRFN_CONCAT;
    std::vector<int> operands;
    if (is_concat) operands = te.nodes[node].parts;
    else if (kind == Node::ISNULL || kind == Node::LIKE || kind == Node::TOBOOL || kind == Node::XCAST || kind == Node::STRFN || kind == Node::TPART || kind == Node::TTRUNC) operands.push_back(te.nodes[node].l);
    for (int l : operands) {
      fit_subtree(ctx, work, wcols, te, l, strict, false);
      if (te.nodes[l].kind != Node::COL && !(is_concat && te.nodes[l].kind == Node::CONST)) materialize_node(ctx, work, wcols, te, l);
    }
  }
  const Node n = te.nodes[node];   // (a copy: evaluate_case appends to te.nodes)
  Column c = kind == Node::CASE    ? evaluate_case(ctx, work, wcols, te, node, strict)
             : kind == Node::STRFN ? evaluate_strfn(ctx, work, te, n)
             : kind == Node::XCAST ? evaluate_cast(ctx, work, te, n)
             : kind == Node::TPART || kind == Node::TTRUNC ? evaluate_temporal(ctx, work, te, n)
                                   : evaluate_bool_op(ctx, work, te, n);
  replace_by_column(work, wcols, te, node, std::move(c));
}

void fit_subtree(Context& ctx, Batch& work, std::vector<PlanColumn>& wcols, TypedExpr& te, int node, bool strict, bool is_root) {
  if (is_typed_op(te, node)) { materialize_typed_op(ctx, work, wcols, te, node, strict); return; }
  if (is_leaf_node(te.nodes[node])) return;
  const int l = te.nodes[node].l, r = te.nodes[node].r;
  if (l >= 0) fit_subtree(ctx, work, wcols, te, l, strict, false);
  if (r >= 0) fit_subtree(ctx, work, wcols, te, r, strict, false);
  if (strict) { if (!is_root) materialize_node(ctx, work, wcols, te, node); return; }
  if (lowers_alone(te, node, wcols)) return;
  // both children fit on their own but not together with this node: turn them into columns, left first
  if (l >= 0 && !is_leaf_node(te.nodes[l])) materialize_node(ctx, work, wcols, te, l);
  if (!lowers_alone(te, node, wcols) && r >= 0 && !is_leaf_node(te.nodes[r])) materialize_node(ctx, work, wcols, te, r);
}

}  // namespace

// true: the sub-tree at `node` lowers into ONE device program
bool lowers_alone(const TypedExpr& te, int node, const std::vector<PlanColumn>& wcols) {
  try {
    Lowered trial;
    lower_expr(te, node, wcols, trial);
    return (int)trial.prog.size() + 1 <= MAX_INSTR;   // room for the STORE of a materialisation
  } catch (const ChqError& e) {
    if (e.code == CHQ_INTERNAL_PROGRAM_LIMIT) return false;
    throw;
  }
}

// After this call lower_expr(te, te.root) succeeds.  `work` / `wcols` start as copies of the batch and its plan columns.
void fit_to_device(Context& ctx, const Batch& rec, const std::vector<PlanColumn>& pcols, const TypedExpr& original,
                   Batch& work, std::vector<PlanColumn>& wcols, TypedExpr& te) {
  for (int pass = 0; pass < 2; ++pass) {
    work = rec; wcols = pcols; te = original;
    try {
      fit_subtree(ctx, work, wcols, te, te.root, /*strict=*/pass == 1, true);
      return;
    } catch (const ChqError& e) {
      const bool data_error = e.code == CHQ_ERR_ARROW_ARITHMETIC_OVERFLOW || e.code == CHQ_ERR_ARROW_DIVIDE_BY_ZERO || e.code == CHQ_ERR_ARROW_CAST;
      if (pass == 1 || !data_error) throw;   // strict order reports the reference's first error
    }
  }
}

}  // namespace chq
