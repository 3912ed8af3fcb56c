// plan.hpp -- host-side expression tree, typing and lowering.
//
// Mirrors what the reference decides on the host for every batch before it touches data:
//   literal typing          RU/compute_value.rs:219-265
//   column / alias lookup   RU/compute_value.rs:266-337
//   binary-op coercion      RU/compute_value.rs:350-461 (get_common_type / cast_to_common_type)
//   scalar flag             RU/compute_value.rs:34-55   (ArrayDatum::new_binary_op)
// and the static checks of the arrow-rs 53 kernels it calls (same-type requirement, length rules).
// The typed tree is then lowered into the accumulator-machine program of device_program.h.
#pragma once
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "../../include/chq.h"
#include "device_program.h"
#include "like_device.h"
#include "strfn_device.h"
#include "case_device.h"
#include "cast_device.h"
#include "temporal_device.h"

namespace chq {

struct ChqError {
  int code;
  std::string msg;
};
// internal: the expression is fine but does not fit ONE device program (instruction / column / temporary limits of
// device_program.h).  The engine reacts by evaluating sub-trees into temporary columns; at the C ABI it never appears.
constexpr int CHQ_INTERNAL_PROGRAM_LIMIT = 1030;

// ---- sqlparser::ast::Expr mirror -----------------------------------------------------------------
struct Expr {
  // LIKE: l = the operand, r = the pattern (a STRING; null when the caller's pattern was not a string literal), flag = NOT
  // LIKE, op = the ESCAPE byte or -1.  ISNULL: l = the operand, flag = IS NOT NULL.  FUNCTION: text = the name as written,
  // args = the arguments (a scalar string function, strfn_device.h, or coalesce / nullif; any other name answers like OTHER
  // "Function(name)").  CASE: l = the operand of a simple CASE or null, args = the n conditions (simple CASE: the values)
  // followed by the n results, r = the ELSE or null.  IN_LIST: l = the operand, args = the list, flag = NOT IN.  BETWEEN:
  // l = the operand, args = {low, high}, flag = NOT BETWEEN.  CAST: l = the operand, op = the chq_cast_type, flag = TRY_CAST.
  // TYPED_STRING (`DATE '..'`, `TIMESTAMP '..'`): op = the chq_typed_string_kind, text = the string.
  enum Kind { NESTED, BINARY, NUMBER, BOOLEAN, STRING, VALUE_OTHER, IDENT, COMPOUND, OTHER, LIKE, ISNULL, FUNCTION, CASE, IN_LIST, BETWEEN, CAST, TYPED_STRING } kind;
  int op = 0;             // chq_binary_operator
  std::string text;       // number text / identifier / string bytes / debug text
  bool flag = false;      // is_long / boolean value / negated
  std::vector<std::string> parts;
  std::unique_ptr<Expr> l, r;
  std::vector<std::unique_ptr<Expr>> args;
};
}  // namespace chq
struct chq_expr { chq::Expr e; };   // the C ABI's expression handle (capi_expr.cpp builds them)
namespace chq {

const char* dtype_name(DType t);
int dtype_width(DType t);   // bytes of a fixed-width value (0 for bool / utf8)
const char* dtype_format(DType t);   // Arrow C format string ("" for T_FIXED_OPAQUE: its column's own)

// A column as the planner sees it
struct PlanColumn {
  std::string name;
  DType type;
  bool has_nulls;
  std::vector<std::string> aliases;
  bool alias_entry_present;   // table_aliases vec has an entry for this column
  std::string format;         // Arrow C format string: decides DataType equality of temporal / decimal columns
  int width = 0;              // bytes per value of a fixed-width column
};

struct Scalar {
  DType type = T_BOOL;
  uint64_t bits = 0;          // value bits (sign-extended ints, IEEE bits for floats, 0/1 for bool)
  std::string str;            // utf8
  bool null = false;          // a Utf8 -> Boolean cast of a literal can make one (arrow-cast: bad spelling = NULL), a failing TRY_CAST, nullif
};

// arrow-cast 53 cast_utf8_to_boolean on one value: 1 / 0, or -1 when the spelling is not a boolean (= NULL, safe cast)
int utf8_to_bool(const uint8_t* bytes, int64_t len);
// how a temporal / decimal column compares with another of the SAME DataType: as I32 / I64 values, as 128-bit integers
// (T_FIXED_OPAQUE returned, width 16), or not at all in this build (T_NTYPES)
DType opaque_compare_class(const PlanColumn& c);
// the TemporalKind of an Arrow format string (Date32 / Date64 / Timestamp / Time32 / Time64), or -1; *zone = a Timestamp's time zone
int temporal_kind_of(const std::string& format, std::string* zone);
extern const char* const kTemporalFieldNames[TF_NFIELDS];
extern const char* const kTemporalUnitNames[TU_NUNITS];

struct Node {
  // (a CMP whose `from` is T_FIXED_OPAQUE compares two Decimal128 columns, a TOBOOL whose `from` is T_UTF8 parses a Utf8
  // column: neither runs inside a device program -- the engine evaluates them into temporary Boolean columns first.  So do
  // LIKE (l = the Utf8 operand, `like` = the compiled pattern, op = 1 for NOT LIKE) and ISNULL (l = the operand, op = 1 for
  // IS NOT NULL): like.hip and typed_ops.hip.  STRFN is a scalar string function (op = its StrFn, l = the Utf8 operand; for
  // STRFN_CONCAT `parts` = the 2..STRFN_MAX_PARTS operands of a flattened `a || b || ..` chain and l = r = -1; for
  // STRFN_SUBSTRING sub_*): strfn.hip writes a temporary Utf8 or Int32 column.  CASE (searched CASE, and what types to it:
  // simple CASE, coalesce, nullif) has op = n WHENs, 1..CASE_MAX_WHENS, `parts` = the n Boolean conditions, the n results and
  // -- case_else -- the ELSE, every result of the node's type, l = r = -1: case.hip writes a temporary column of that type.
  // A result may be a CONST whose cval is null, of any type (nullif).  fmt_col: the batch column whose Arrow format a
  // T_FIXED_OPAQUE result has (a COL's is its own).  XCAST is an explicit CAST / TRY_CAST (l = the operand, `from` its type,
  // `type` the target, op = 1 for TRY_CAST): cast.hip writes a temporary column of the target type.  CAST stays the implicit
  // widening of the coercion table, an instruction of the device program.  TPART is EXTRACT / date_part (l = the temporal
  // operand, a column or a TTRUNC; op = the TemporalField; tkind = the operand's TemporalKind; the result is Int32), TTRUNC is
  // date_trunc (op = the TemporalUnit; the result is T_FIXED_OPAQUE with the operand's format, fmt_col): temporal.hip writes a
  // temporary column.  A CONST with `tlit` set is a DATE / TIMESTAMP literal that has not met its temporal neighbour yet (tlit =
  // chq_typed_string_kind + 1, cval.str = the string); binary() turns it into an Int32 / Int64 CONST of the neighbour's unit,
  // fmt_col = the neighbour's column, and nothing else accepts one.)
  enum Kind { COL, CONST, ARITH, CMP, ANDOR, CAST, TOBOOL, LIKE, ISNULL, STRFN, CASE, XCAST, TPART, TTRUNC } kind;
  DType type;
  bool is_scalar;   // ArrayDatum.is_scalar
  bool len1;        // array length is 1 regardless of the batch (built from literals only)
  int col = -1;     // COL
  Scalar cval;      // CONST
  int op = 0;       // ARITH: OP_ADD..OP_REM, CMP: OP_EQ..OP_GE, ANDOR: OP_AND/OP_OR
  int l = -1, r = -1;
  int ref_order = 0;
  DType from = T_BOOL;  // CAST / TOBOOL source type
  std::shared_ptr<const LikePattern> like;   // LIKE
  std::vector<int> parts;                    // STRFN_CONCAT, CASE
  bool case_else = false;                    // CASE
  int fmt_col = -1;                          // CASE / TTRUNC / temporal literal of T_FIXED_OPAQUE
  int tkind = 0;                             // TPART, TTRUNC: TemporalKind of the operand
  int tlit = 0;                              // CONST: an unresolved DATE / TIMESTAMP literal
  TemporalLiteral tval{};                    // .. as it was parsed where it stands
  int32_t sub_p = 0, sub_cnt = 0;            // STRFN_SUBSTRING: FROM sub_p [FOR sub_cnt]
  bool sub_has_cnt = false;
  // every operand: l, r and the parts
  template <class F> void each_child(F f) const { if (l >= 0) f(l); if (r >= 0) f(r); for (int c : parts) f(c); }
};

struct TypedExpr {
  std::vector<Node> nodes;
  int root = -1;
  // A static error (type / lookup / literal-folding error) met while walking the tree.  The reference would
  // already have evaluated every subtree completed before that point, so a data-dependent error (integer
  // overflow, division by zero) in one of `validate_roots` wins over it; the engine checks them first.
  int pending_code = 0;
  std::string pending_msg;
  std::vector<int> validate_roots;
  const Node& at(int i) const { return nodes[i]; }
};

// Build the typed tree for `e` against the batch columns.  A static error is thrown directly when nothing
// evaluated before it could have failed on data; otherwise it is returned as `pending_*` (see TypedExpr).  `nrows` is needed for the arrow length rules between len-1 arrays and
// columns.  `enable_minus`: accept BinaryOperator::Minus (not implemented by the reference).
TypedExpr type_expr(const Expr& e, const std::vector<PlanColumn>& cols, int64_t nrows, bool enable_minus);

// Evaluate a len-1 (literal-only) subtree on the host with the device kernels' semantics.
// Throws ChqError for arithmetic errors.  `valid` is always true (literals are never null).
Scalar fold_constant(const TypedExpr& t, int node);

// true: the sub-tree at `node` holds checked integer arithmetic on columns, or a CAST (not TRY_CAST) of a column whose
// conversion can fail (cast_can_fail), i.e. it can fail on data
bool has_checked_arith(const TypedExpr& t, int node);
// CASE node `node`: guard[j] = operand parts[j] is evaluated under a guard (the lazy-error rule): it
// can fail on data and is not the first condition, which every row evaluates.  Returns how many are.
int case_guarded_parts(const TypedExpr& t, int node, std::vector<char>* guard);

// Lowered program (host form; engine patches column pointers in)
struct Lowered {
  std::vector<Instr> prog;
  std::vector<int> refs;              // batch column index per ColRef slot
  std::vector<std::string> strs;      // scalar strings referenced by OP_STRCMP
  int num_temps = 0;                  // numeric temporaries used
  bool wide = false;                  // needs 64-bit value classes
};

// Append code that leaves the value of `node` in the accumulator. Throws CHQ_ERR_NOT_SUPPORTED when
// the expression exceeds the machine's limits (documented in DESIGN.md).
void lower_expr(const TypedExpr& t, int node, const std::vector<PlanColumn>& cols, Lowered& out);

}  // namespace chq
