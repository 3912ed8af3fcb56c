// The expression-handle constructors of the C ABI alone, under the host sanitizers (tests/test_capi_args_host.py builds
// and runs this).  Every node kind is built and every field of the result checked; every constructor that takes children is
// handed a null in each position in turn, with the other handles live, and must refuse.  AddressSanitizer's leak report at
// exit shows that every refusing path freed every handle it owned, AddressSanitizer itself that none was freed twice.
#include "../chapterhouseqe_amd/csrc/capi_expr.cpp"

#include <cstdio>
#include <cstring>
#include <string>

static long n_checks = 0, n_bad = 0;
#define CHECK(cond) do { ++n_checks; if (!(cond)) { ++n_bad; fprintf(stderr, "line %d: %s\n", __LINE__, #cond); } } while (0)

static chq_expr* leaf(int i) { return chq_expr_number(std::to_string(i).c_str(), 0); }
// `e` is a NUMBER leaf made by leaf(i)
static bool is_leaf(const std::unique_ptr<Expr>& e, int i) { return e && e->kind == Expr::NUMBER && e->text == std::to_string(i) && !e->l && !e->r && e->args.empty(); }
// nothing set but what the caller names
static bool bare(const chq_expr* h, bool l, bool r, size_t nargs) {
  return h && (h->e.l != nullptr) == l && (h->e.r != nullptr) == r && h->e.args.size() == nargs && h->e.parts.empty();
}

static void leaves() {
  chq_expr* h = chq_expr_identifier("id");
  CHECK(bare(h, false, false, 0) && h->e.kind == Expr::IDENT && h->e.text == "id" && !h->e.flag && h->e.op == 0);
  chq_expr_free(h);
  h = chq_expr_identifier(nullptr);
  CHECK(bare(h, false, false, 0) && h->e.kind == Expr::IDENT && h->e.text.empty());
  chq_expr_free(h);
  const char* parts[3] = {"t", nullptr, "c"};
  h = chq_expr_compound_identifier(parts, 3);
  CHECK(h && h->e.kind == Expr::COMPOUND && h->e.parts.size() == 3 && h->e.parts[0] == "t" && h->e.parts[1].empty() && h->e.parts[2] == "c");
  CHECK(h && !h->e.l && !h->e.r && h->e.args.empty() && h->e.text.empty());
  chq_expr_free(h);
  h = chq_expr_compound_identifier(nullptr, 0);
  CHECK(bare(h, false, false, 0) && h->e.kind == Expr::COMPOUND);
  chq_expr_free(h);
  h = chq_expr_compound_identifier(parts, -1);
  CHECK(bare(h, false, false, 0) && h->e.kind == Expr::COMPOUND);
  chq_expr_free(h);
  CHECK(chq_expr_compound_identifier(nullptr, 2) == nullptr);   // (null parts with a count: refused, not read)
  h = chq_expr_number("12", 1);
  CHECK(bare(h, false, false, 0) && h->e.kind == Expr::NUMBER && h->e.text == "12" && h->e.flag);
  chq_expr_free(h);
  h = chq_expr_number(nullptr, 0);
  CHECK(bare(h, false, false, 0) && h->e.kind == Expr::NUMBER && h->e.text.empty() && !h->e.flag);
  chq_expr_free(h);
  h = chq_expr_boolean(7);
  CHECK(bare(h, false, false, 0) && h->e.kind == Expr::BOOLEAN && h->e.flag && h->e.text.empty());
  chq_expr_free(h);
  h = chq_expr_boolean(0);
  CHECK(bare(h, false, false, 0) && h->e.kind == Expr::BOOLEAN && !h->e.flag);
  chq_expr_free(h);
  h = chq_expr_single_quoted_string("a\0bc", 3);
  CHECK(bare(h, false, false, 0) && h->e.kind == Expr::STRING && h->e.text == std::string("a\0b", 3));
  chq_expr_free(h);
  h = chq_expr_single_quoted_string(nullptr, 3);
  CHECK(bare(h, false, false, 0) && h->e.kind == Expr::STRING && h->e.text.empty());
  chq_expr_free(h);
  h = chq_expr_single_quoted_string("abc", 0);
  CHECK(bare(h, false, false, 0) && h->e.kind == Expr::STRING && h->e.text.empty());
  chq_expr_free(h);
  h = chq_expr_single_quoted_string("abc", -2);
  CHECK(bare(h, false, false, 0) && h->e.kind == Expr::STRING && h->e.text.empty());
  chq_expr_free(h);
  h = chq_expr_unsupported_value("Null");
  CHECK(bare(h, false, false, 0) && h->e.kind == Expr::VALUE_OTHER && h->e.text == "Null");
  chq_expr_free(h);
  h = chq_expr_unsupported_value(nullptr);
  CHECK(bare(h, false, false, 0) && h->e.kind == Expr::VALUE_OTHER && h->e.text.empty());
  chq_expr_free(h);
  h = chq_expr_unsupported("Exists");
  CHECK(bare(h, false, false, 0) && h->e.kind == Expr::OTHER && h->e.text == "Exists");
  chq_expr_free(h);
  h = chq_expr_unsupported(nullptr);
  CHECK(bare(h, false, false, 0) && h->e.kind == Expr::OTHER && h->e.text.empty());
  chq_expr_free(h);
  chq_expr_free(nullptr);
}

static void singles() {
  chq_expr* h = chq_expr_binary_op(leaf(1), CHQ_BINOP_PLUS, "Plus", leaf(2));
  CHECK(bare(h, true, true, 0) && h->e.kind == Expr::BINARY && h->e.op == (int)CHQ_BINOP_PLUS && h->e.text == "Plus" && !h->e.flag);
  CHECK(h && is_leaf(h->e.l, 1) && is_leaf(h->e.r, 2));
  chq_expr_free(h);
  h = chq_expr_binary_op(leaf(1), CHQ_BINOP_GT, nullptr, leaf(2));
  CHECK(bare(h, true, true, 0) && h->e.op == (int)CHQ_BINOP_GT && h->e.text.empty());
  chq_expr_free(h);
  CHECK(chq_expr_binary_op(nullptr, CHQ_BINOP_PLUS, "Plus", leaf(2)) == nullptr);
  CHECK(chq_expr_binary_op(leaf(1), CHQ_BINOP_PLUS, "Plus", nullptr) == nullptr);
  CHECK(chq_expr_binary_op(nullptr, CHQ_BINOP_PLUS, "Plus", nullptr) == nullptr);

  h = chq_expr_nested(leaf(3));
  CHECK(bare(h, true, false, 0) && h->e.kind == Expr::NESTED && is_leaf(h->e.l, 3) && h->e.text.empty() && !h->e.flag && h->e.op == 0);
  chq_expr_free(h);
  CHECK(chq_expr_nested(nullptr) == nullptr);

  h = chq_expr_like(leaf(4), "a%\0_", 4, 1, 'x');
  CHECK(bare(h, true, true, 0) && h->e.kind == Expr::LIKE && is_leaf(h->e.l, 4) && h->e.flag && h->e.op == 'x');
  CHECK(h && h->e.r->kind == Expr::STRING && h->e.r->text == std::string("a%\0_", 4) && !h->e.r->l && !h->e.r->r && h->e.r->args.empty());
  chq_expr_free(h);
  h = chq_expr_like(leaf(4), "abc", 0, 0, -5);
  CHECK(bare(h, true, true, 0) && !h->e.flag && h->e.op == -1 && h->e.r->kind == Expr::STRING && h->e.r->text.empty());
  chq_expr_free(h);
  h = chq_expr_like(leaf(4), nullptr, 3, 0, -1);   // a pattern that was no string literal: r stays empty
  CHECK(bare(h, true, false, 0) && h->e.kind == Expr::LIKE && is_leaf(h->e.l, 4) && h->e.op == -1);
  chq_expr_free(h);
  CHECK(chq_expr_like(nullptr, "a", 1, 0, -1) == nullptr);

  h = chq_expr_is_null(leaf(5), 1);
  CHECK(bare(h, true, false, 0) && h->e.kind == Expr::ISNULL && is_leaf(h->e.l, 5) && h->e.flag && h->e.op == 0);
  chq_expr_free(h);
  h = chq_expr_is_null(leaf(5), 0);
  CHECK(bare(h, true, false, 0) && !h->e.flag);
  chq_expr_free(h);
  CHECK(chq_expr_is_null(nullptr, 0) == nullptr);

  h = chq_expr_cast(leaf(6), CHQ_CAST_OTHER, 1);
  CHECK(bare(h, true, false, 0) && h->e.kind == Expr::CAST && is_leaf(h->e.l, 6) && h->e.flag && h->e.op == (int)CHQ_CAST_OTHER);
  chq_expr_free(h);
  h = chq_expr_cast(leaf(6), (chq_cast_type)0, 0);
  CHECK(bare(h, true, false, 0) && !h->e.flag && h->e.op == 0);
  chq_expr_free(h);
  CHECK(chq_expr_cast(nullptr, CHQ_CAST_OTHER, 0) == nullptr);

  h = chq_expr_between(leaf(7), 1, leaf(8), leaf(9));
  CHECK(bare(h, true, false, 2) && h->e.kind == Expr::BETWEEN && h->e.flag && is_leaf(h->e.l, 7) && is_leaf(h->e.args[0], 8) && is_leaf(h->e.args[1], 9));
  chq_expr_free(h);
  h = chq_expr_between(leaf(7), 0, leaf(8), leaf(9));
  CHECK(bare(h, true, false, 2) && !h->e.flag);
  chq_expr_free(h);
  CHECK(chq_expr_between(nullptr, 0, leaf(8), leaf(9)) == nullptr);
  CHECK(chq_expr_between(leaf(7), 0, nullptr, leaf(9)) == nullptr);
  CHECK(chq_expr_between(leaf(7), 0, leaf(8), nullptr) == nullptr);
}

// a list of three live handles, `missing` (0..2) left null
struct List3 {
  chq_expr* h[3];
  explicit List3(int missing = -1, int base = 10) { for (int i = 0; i < 3; ++i) h[i] = i == missing ? nullptr : leaf(base + i); }
  void free_all() { for (chq_expr*& x : h) { chq_expr_free(x); x = nullptr; } }   // when no constructor took them
};

static void lists() {
  // ---- FUNCTION
  { List3 a;
    chq_expr* h = chq_expr_function("Upper", a.h, 3);
    CHECK(bare(h, false, false, 3) && h->e.kind == Expr::FUNCTION && h->e.text == "Upper" && !h->e.flag && h->e.op == 0);
    CHECK(h && is_leaf(h->e.args[0], 10) && is_leaf(h->e.args[1], 11) && is_leaf(h->e.args[2], 12));
    chq_expr_free(h); }
  { chq_expr* h = chq_expr_function("now", nullptr, 0);
    CHECK(bare(h, false, false, 0) && h->e.kind == Expr::FUNCTION && h->e.text == "now");
    chq_expr_free(h); }
  { List3 a; CHECK(chq_expr_function(nullptr, a.h, 3) == nullptr); }   // no name: refuses and frees the arguments
  for (int i = 0; i < 3; ++i) { List3 a(i); CHECK(chq_expr_function("f", a.h, 3) == nullptr); }
  CHECK(chq_expr_function("f", nullptr, 3) == nullptr);
  { List3 a; CHECK(chq_expr_function("f", a.h, -1) == nullptr); a.free_all(); }   // (a negative count names no handle to take)

  // ---- IN_LIST
  { List3 a;
    chq_expr* h = chq_expr_in_list(leaf(1), a.h, 3, 1);
    CHECK(bare(h, true, false, 3) && h->e.kind == Expr::IN_LIST && h->e.flag && is_leaf(h->e.l, 1) && h->e.text.empty() && h->e.op == 0);
    CHECK(h && is_leaf(h->e.args[0], 10) && is_leaf(h->e.args[1], 11) && is_leaf(h->e.args[2], 12));
    chq_expr_free(h); }
  { chq_expr* h = chq_expr_in_list(leaf(1), nullptr, 0, 0);
    CHECK(bare(h, true, false, 0) && h->e.kind == Expr::IN_LIST && !h->e.flag);
    chq_expr_free(h); }
  { List3 a; CHECK(chq_expr_in_list(nullptr, a.h, 3, 0) == nullptr); }
  for (int i = 0; i < 3; ++i) { List3 a(i); CHECK(chq_expr_in_list(leaf(1), a.h, 3, 0) == nullptr); }
  CHECK(chq_expr_in_list(leaf(1), nullptr, 3, 0) == nullptr);
  { List3 a; CHECK(chq_expr_in_list(leaf(1), a.h, -1, 0) == nullptr); a.free_all(); }

  // ---- CASE: args = the conditions, then the results; operand and ELSE may be absent
  { List3 c(-1, 10), r(-1, 20);
    chq_expr* h = chq_expr_case(leaf(1), c.h, r.h, 3, leaf(2));
    CHECK(bare(h, true, true, 6) && h->e.kind == Expr::CASE && is_leaf(h->e.l, 1) && is_leaf(h->e.r, 2) && !h->e.flag && h->e.op == 0 && h->e.text.empty());
    for (int i = 0; i < 3; ++i) CHECK(h && is_leaf(h->e.args[(size_t)i], 10 + i) && is_leaf(h->e.args[(size_t)i + 3], 20 + i));
    chq_expr_free(h); }
  { List3 c(-1, 10), r(-1, 20);
    chq_expr* h = chq_expr_case(nullptr, c.h, r.h, 1, nullptr);   // (one WHEN of the three: the lists' other handles stay the caller's)
    CHECK(bare(h, false, false, 2) && h->e.kind == Expr::CASE && is_leaf(h->e.args[0], 10) && is_leaf(h->e.args[1], 20));
    chq_expr_free(h);
    c.h[0] = r.h[0] = nullptr; c.free_all(); r.free_all(); }
  { List3 c(-1, 10), r(-1, 20);
    chq_expr* h = chq_expr_case(leaf(1), c.h, r.h, 3, nullptr);
    CHECK(bare(h, true, false, 6));
    chq_expr_free(h); }
  { List3 c(-1, 10), r(-1, 20);
    chq_expr* h = chq_expr_case(nullptr, c.h, r.h, 3, leaf(2));
    CHECK(bare(h, false, true, 6));
    chq_expr_free(h); }
  for (int i = 0; i < 3; ++i) {
    { List3 c(i, 10), r(-1, 20); CHECK(chq_expr_case(leaf(1), c.h, r.h, 3, leaf(2)) == nullptr); }
    { List3 c(-1, 10), r(i, 20); CHECK(chq_expr_case(leaf(1), c.h, r.h, 3, leaf(2)) == nullptr); }
  }
  { List3 r(-1, 20); CHECK(chq_expr_case(leaf(1), nullptr, r.h, 3, leaf(2)) == nullptr); }
  { List3 c(-1, 10); CHECK(chq_expr_case(leaf(1), c.h, nullptr, 3, leaf(2)) == nullptr); }
  CHECK(chq_expr_case(leaf(1), nullptr, nullptr, 3, leaf(2)) == nullptr);
  { List3 c(-1, 10), r(-1, 20);
    CHECK(chq_expr_case(leaf(1), c.h, r.h, -1, leaf(2)) == nullptr);
    CHECK(chq_expr_case(leaf(1), c.h, r.h, 0, leaf(2)) == nullptr);   // a CASE has at least one WHEN
    c.free_all(); r.free_all(); }
  CHECK(chq_expr_case(nullptr, nullptr, nullptr, 0, leaf(2)) == nullptr);
}

static void deep() {
  const int depth = 400;
  chq_expr* h = leaf(0);
  for (int i = 1; i <= depth && h; ++i) h = (i & 1) ? chq_expr_nested(h) : chq_expr_binary_op(h, CHQ_BINOP_PLUS, "Plus", leaf(i));
  CHECK(h != nullptr);
  int seen = 0;
  for (const Expr* e = h ? &h->e : nullptr; e && e->l; e = e->l.get()) ++seen;
  CHECK(seen == depth);
  chq_expr_free(h);
}

int main() {
  leaves();
  singles();
  lists();
  deep();
  printf("%ld checks, %ld mismatches\n", n_checks, n_bad);
  return n_bad ? 1 : 0;
}
