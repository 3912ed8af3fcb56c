// capi_expr.cpp -- the expression-handle constructors of include/chq.h.  They build the Expr tree of plan.hpp and need
// nothing of the engine.  A constructor that takes child handles owns them from the call on: it adopts all of them, or --
// when one is missing, a list is malformed or memory ran out -- frees all of them and returns nullptr.
#include <initializer_list>
#include <new>

#include "plan.hpp"

using namespace chq;

namespace {

chq_expr* new_expr(Expr::Kind k) { chq_expr* e = new (std::nothrow) chq_expr(); if (e) e->e.kind = k; return e; }
const char* text_or_empty(const char* s) { return s ? s : ""; }

// the wrapper structs own nothing but the Expr: move the tree in and drop the shell
std::unique_ptr<Expr> adopt(chq_expr* child) {
  std::unique_ptr<Expr> tree(new Expr(std::move(child->e)));
  delete child;
  return tree;
}

// the list half: moves `n` handles into e->args; false -- and every handle freed -- when `e` or one of them is missing
bool take_children(chq_expr* e, chq_expr* const* list, int n) {
  bool ok = e && n >= 0 && (list || n == 0);
  for (int i = 0; ok && i < n; ++i) ok = list[i] != nullptr;
  if (!ok) { for (int i = 0; list && i < n; ++i) chq_expr_free(list[i]); return false; }
  for (int i = 0; i < n; ++i) e->e.args.push_back(adopt(list[i]));
  return true;
}

// a single child and where it goes: Expr::l, Expr::r, or (no slot) the end of Expr::args; `optional`: may be null
struct Child { chq_expr* handle; std::unique_ptr<Expr> Expr::*slot; bool optional; };
struct ChildList { chq_expr* const* items; int n; };

// `e` with every child adopted (the lists first, in order, then the singles), or everything freed -- `e` included -- and
// nullptr.  A null `e` refuses: a constructor with a condition of its own passes nullptr instead of a fresh node.
chq_expr* adopt_all(chq_expr* e, std::initializer_list<Child> singles, std::initializer_list<ChildList> lists = {}) {
  bool ok = e != nullptr;
  for (const Child& c : singles) ok = ok && (c.handle || c.optional);
  for (const ChildList& l : lists) ok = take_children(ok ? e : nullptr, l.items, l.n) && ok;
  if (!ok) {
    for (const Child& c : singles) chq_expr_free(c.handle);
    delete e;   // (with the lists it had taken before one was refused)
    return nullptr;
  }
  for (const Child& c : singles) {
    if (!c.handle) continue;
    if (c.slot) e->e.*c.slot = adopt(c.handle);
    else e->e.args.push_back(adopt(c.handle));
  }
  return e;
}

}  // namespace

extern "C" {

chq_expr* chq_expr_identifier(const char* name) { chq_expr* e = new_expr(Expr::IDENT); if (e) e->e.text = text_or_empty(name); return e; }
chq_expr* chq_expr_compound_identifier(const char* const* parts, int n) {
  if (!parts && n > 0) return nullptr;
  chq_expr* e = new_expr(Expr::COMPOUND);
  if (e) for (int i = 0; i < n; ++i) e->e.parts.push_back(text_or_empty(parts[i]));
  return e;
}
chq_expr* chq_expr_number(const char* text, int is_long) {
  chq_expr* e = new_expr(Expr::NUMBER);
  if (e) { e->e.text = text_or_empty(text); e->e.flag = is_long != 0; }
  return e;
}
chq_expr* chq_expr_boolean(int value) { chq_expr* e = new_expr(Expr::BOOLEAN); if (e) e->e.flag = value != 0; return e; }
chq_expr* chq_expr_single_quoted_string(const char* bytes, int64_t len) {
  chq_expr* e = new_expr(Expr::STRING);
  if (e && bytes && len > 0) e->e.text.assign(bytes, (size_t)len);
  return e;
}
chq_expr* chq_expr_unsupported_value(const char* debug) { chq_expr* e = new_expr(Expr::VALUE_OTHER); if (e) e->e.text = text_or_empty(debug); return e; }
chq_expr* chq_expr_unsupported(const char* debug) { chq_expr* e = new_expr(Expr::OTHER); if (e) e->e.text = text_or_empty(debug); return e; }
void chq_expr_free(chq_expr* e) { delete e; }

chq_expr* chq_expr_binary_op(chq_expr* left, chq_binary_operator op, const char* op_debug, chq_expr* right) {
  chq_expr* e = adopt_all(new_expr(Expr::BINARY), {{left, &Expr::l, false}, {right, &Expr::r, false}});
  if (e) { e->e.op = (int)op; e->e.text = text_or_empty(op_debug); }
  return e;
}
chq_expr* chq_expr_nested(chq_expr* inner) { return adopt_all(new_expr(Expr::NESTED), {{inner, &Expr::l, false}}); }
chq_expr* chq_expr_like(chq_expr* operand, const char* pattern, int64_t pattern_len, int negated, int escape) {
  chq_expr* e = adopt_all(new_expr(Expr::LIKE), {{operand, &Expr::l, false}});
  if (!e) return nullptr;
  if (pattern) {   // (null: the caller's pattern was not a string literal -- typing reports it)
    e->e.r.reset(new Expr());
    e->e.r->kind = Expr::STRING;
    if (pattern_len > 0) e->e.r->text.assign(pattern, (size_t)pattern_len);
  }
  e->e.flag = negated != 0; e->e.op = escape < 0 ? -1 : escape;
  return e;
}
chq_expr* chq_expr_is_null(chq_expr* operand, int negated) {
  chq_expr* e = adopt_all(new_expr(Expr::ISNULL), {{operand, &Expr::l, false}});
  if (e) e->e.flag = negated != 0;
  return e;
}
chq_expr* chq_expr_function(const char* name, chq_expr* const* args, int n_args) {
  chq_expr* e = adopt_all(name ? new_expr(Expr::FUNCTION) : nullptr, {}, {{args, n_args}});
  if (e) e->e.text = name;
  return e;
}
chq_expr* chq_expr_case(chq_expr* operand, chq_expr* const* conditions, chq_expr* const* results, int n_when, chq_expr* else_result) {
  return adopt_all(n_when >= 1 ? new_expr(Expr::CASE) : nullptr, {{operand, &Expr::l, true}, {else_result, &Expr::r, true}},
                   {{conditions, n_when}, {results, n_when}});
}
chq_expr* chq_expr_in_list(chq_expr* expr, chq_expr* const* list, int n, int negated) {
  chq_expr* e = adopt_all(new_expr(Expr::IN_LIST), {{expr, &Expr::l, false}}, {{list, n}});
  if (e) e->e.flag = negated != 0;
  return e;
}
chq_expr* chq_expr_between(chq_expr* expr, int negated, chq_expr* low, chq_expr* high) {
  chq_expr* e = adopt_all(new_expr(Expr::BETWEEN), {{expr, &Expr::l, false}, {low, nullptr, false}, {high, nullptr, false}});
  if (e) e->e.flag = negated != 0;
  return e;
}
chq_expr* chq_expr_cast(chq_expr* operand, chq_cast_type to, int try_cast) {
  chq_expr* e = adopt_all(new_expr(Expr::CAST), {{operand, &Expr::l, false}});
  if (e) { e->e.op = (int)to; e->e.flag = try_cast != 0; }
  return e;
}
chq_expr* chq_expr_typed_string(chq_typed_string_kind kind, const char* bytes, int64_t len) {
  chq_expr* e = new_expr(Expr::TYPED_STRING);
  if (e) { e->e.op = (int)kind; if (bytes && len > 0) e->e.text.assign(bytes, (size_t)len); }
  return e;
}

}  // extern "C"
