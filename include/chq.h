/*
 * chq.h -- C ABI of the MI355X-native filter / projection record kernels for ChapterhouseDB.
 *
 * This is the drop-in boundary for ONE path of the reference (alekLukanen/ChapterhouseQE): the
 * record_utils functions its `filter` and `materialize` operator tasks call once per RecordBatch.
 * Reference paths are relative to the reference repo root; RU = src/handlers/operator_handler/
 * operators/record_utils.
 *
 *   chq_filter_record   replaces  RU/filter_record.rs:21-25    pub fn filter_record(rec, table_aliases, expr)
 *                        called at operators/filter_tasks/filter_task.rs:99
 *   chq_project_record  replaces  RU/record_projection.rs:16-20 pub fn project_record(fields, record, table_aliases)
 *                        called at operators/materialize_tasks/materialize_files_task.rs:110
 *   chq_compute_value   replaces  RU/compute_value.rs:57-61     pub fn compute_value(rec, table_aliases, expr)
 *   chq_expr_*          carry     sqlparser::ast::Expr  (the variants RU/compute_value.rs:62-343 matches on)
 *   chq_select_item     carries   sqlparser::ast::SelectItem (RU/record_projection.rs:25-69)
 *   chq_table_aliases   carries   table_aliases: &Vec<Vec<String>> (RU/record_aliases.rs:12-59)
 *   status codes        mirror    ComputeValueError (RU/compute_value.rs:13-32), FilterRecordError
 *                                 (RU/filter_record.rs:12-15), ProjectRecordError (RU/record_projection.rs:11-14)
 *                                 and the ArrowError variants of the arrow-rs 53 kernels behind them.
 *
 * Record batches cross the boundary as Arrow C (Device) Data Interface structs (chq_arrow_abi.h): a
 * struct-typed ArrowDeviceArray with one child per column plus its ArrowSchema.  Inputs may live on
 * the host (ARROW_DEVICE_CPU; the library stages them to HBM) or already on the GPU (ARROW_DEVICE_ROCM,
 * zero copy).  Inputs are borrowed for the duration of the call and never modified or released.
 * Outputs are freshly allocated, owned by the caller and freed through the standard Arrow `release`
 * callbacks; the caller chooses whether they are returned in HBM (stay on the GPU for the next
 * operator) or copied back to host memory.
 *
 * No torch / C++ types appear here.  All functions are thread-safe per context: one chq_ctx per
 * operator instance (the reference runs one batch at a time per instance, filter_task.rs:86-125).
 * Everything is computed by HIP kernels on gfx950; there is no CPU fallback -- a missing or unusable
 * device is an error (CHQ_ERR_DEVICE).
 */
#ifndef CHQ_H
#define CHQ_H

#include <stdint.h>
#include "chq_arrow_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CHQ_ABI_VERSION 1

/* ---- status codes --------------------------------------------------------------------------- */
typedef enum chq_status {
  CHQ_OK = 0,
  /* ComputeValueError, RU/compute_value.rs:13-32 */
  CHQ_ERR_VALUE_TYPE_NOT_IMPLEMENTED = 1,
  CHQ_ERR_EXPRESSION_TYPE_NOT_IMPLEMENTED = 2,
  CHQ_ERR_BINARY_OPERATOR_NOT_IMPLEMENTED = 3,
  CHQ_ERR_BINARY_OPERATION_CAST_FAILED = 4,
  CHQ_ERR_FAILED_TO_PARSE_AS_AN_INTEGER = 5,
  CHQ_ERR_FAILED_TO_PARSE_AS_A_FLOAT = 6,
  CHQ_ERR_COLUMN_NOT_FOUND = 7,
  CHQ_ERR_IDENTIFIER_NOT_FOUND = 8,
  CHQ_ERR_UNSUPPORTED_TYPE_COERSION = 9,
  /* FilterRecordError, RU/filter_record.rs:12-15 */
  CHQ_ERR_CAST_TO_BOOLEAN_ARRAY_FAILED = 10,
  /* ProjectRecordError, RU/record_projection.rs:11-14 */
  CHQ_ERR_PROJECT_NOT_IMPLEMENTED = 11,
  /* ArrowError raised by the arrow-rs kernels the reference calls */
  CHQ_ERR_ARROW_ARITHMETIC_OVERFLOW = 20,
  CHQ_ERR_ARROW_DIVIDE_BY_ZERO = 21,
  CHQ_ERR_ARROW_INVALID_ARGUMENT = 22,
  CHQ_ERR_ARROW_COMPUTE = 23,
  CHQ_ERR_ARROW_CAST = 24,
  /* this implementation */
  CHQ_ERR_NOT_SUPPORTED = 30,   /* valid in the reference, outside this build's scope */
  CHQ_ERR_INVALID_HANDLE = 31,
  CHQ_ERR_DEVICE = 40,          /* HIP runtime / no usable gfx950 device */
  CHQ_ERR_OUT_OF_MEMORY = 41
} chq_status;

/* ---- context -------------------------------------------------------------------------------- */
typedef struct chq_ctx chq_ctx;

/* One context per operator instance.  `hip_stream` is a hipStream_t to run on (pass hipStreamLegacy /
 * hipStreamPerThread for the default streams), or NULL to let the context create its own non-blocking
 * stream -- in that case work the caller issued on other streams must be synchronised by the caller.  Fails with CHQ_ERR_DEVICE when no GPU is usable. */
chq_status chq_ctx_create(int device_id, void* hip_stream, chq_ctx** out);
void chq_ctx_destroy(chq_ctx* ctx);
/* Message of the last failing call on this context (valid until the next call on it). */
const char* chq_ctx_last_error(const chq_ctx* ctx);
/* hipStream_t the context launches on. */
void* chq_ctx_stream(const chq_ctx* ctx);
/* Options: "tile_kind" (-1 auto, 0: 16384-row tiles, 1/2: 2048-row tiles), "enable_minus",
 * "time_kernels", "trim_pool" (return every cached HBM / host block to the system), "host_pool_bytes" (cap of the
 * process-wide cache of host result buffers, default 8 GiB, 0 disables it), "fuse" (chq_filter_project_record's
 * single-pass kernel: 0 never, 1 = default: when it moves clearly fewer bytes than the two steps, 2 whenever the
 * inputs allow), "group_mode" (chq_filter_records layout: 0 auto, 1 per-tile table, 2 wave-packed).  Switches that exist for A/B
 * measurements and tests (all default 1): "fold_utf8" (short-string Utf8 columns inside the main kernel), "group_fold"
 * (the same for batch groups), "group_bits" (validity bitmaps / Boolean columns of a wave-packed device group in the
 * one-launch path), "stash" (-1 auto .. 2 predicate columns kept in LDS between the two phases), "split_rows" (rows from
 * which a batch is launched as complete tiles + tail), "uniform_utf8_rows" (batches of at least this many rows -- default 2^24, 0 = never -- have
 * their Utf8 columns checked for ONE value length and, if so, filtered as fixed-width columns), "parquet_page_rows" (chq_record_to_parquet: rows per data page,
 * default 65 536, rounded to multiples of 4 096; a chunk never gets more than 64 pages), "snappy_blocks" (Parquet scan: 1 = a
 * snappy page of three or more 64 KiB blocks is inflated one wave per BLOCK after a walk of its element chain, 0 = one wave
 * per page, 2 = the blocks give up and the page is redone whole -- the path a stream with blocks that depend on each other
 * takes --, 3 = as 1 but every chain walked by one wave instead of one wave per segment of the page's input; 2 and 3 for tests).
 * Unknown keys fail.
 *
 * Type coverage of expressions = the reference's (RU/compute_value.rs:350-431): the integer / float coercion table,
 * Utf8 and Boolean comparisons, Float16 (widening, f16 arithmetic and comparisons), same-type comparisons of Date32 /
 * Date64 / Time32 / Time64 / Timestamp / Duration / Decimal128 columns, and casts to Boolean under AND / OR from numeric
 * and Utf8 operands (a spelling arrow-cast does not know is NULL).  CHQ_ERR_NOT_SUPPORTED remains for ARITHMETIC on
 * decimals, durations and date / timestamp differences, and for comparisons of FixedSizeBinary / interval columns.
 * Beyond the reference: [NOT] LIKE on Utf8 (chq_expr_like), IS [NOT] NULL on every type (chq_expr_is_null) and the scalar
 * string functions (CHQ_BINOP_STRING_CONCAT, chq_expr_function), whose results are Utf8 or Int32 columns; CASE, coalesce and
 * nullif (chq_expr_case, chq_expr_function), whose result has any of these types; BETWEEN and IN lists (chq_expr_between,
 * chq_expr_in_list); explicit CAST / TRY_CAST between Boolean, the integers, the floats and Utf8 (chq_expr_cast); DATE /
 * TIMESTAMP literals beside Date / Timestamp operands (chq_expr_typed_string), EXTRACT / date_part and date_trunc
 * (chq_expr_function). */
chq_status chq_ctx_set_option(chq_ctx* ctx, const char* key, int64_t value);
/* Counters of the last filter call: rows in, rows out, tiles, kernel launches. */
typedef struct chq_call_stats {
  int64_t rows_in, rows_out, tiles, launches;
  int64_t bytes_read_alg, bytes_written_alg;   /* algorithmic bytes per SURVEY.md section 8(d) */
  int64_t kernel_ns;   /* duration of the main kernel launch(es), HIP events on the context's stream; 0 unless
                          the context option "time_kernels" is set */
} chq_call_stats;
void chq_ctx_last_stats(const chq_ctx* ctx, chq_call_stats* out);

int chq_abi_version(void);
const char* chq_status_name(chq_status s);

/* ---- expressions: sqlparser::ast::Expr ------------------------------------------------------- */
typedef struct chq_expr chq_expr;

/* sqlparser::ast::BinaryOperator; arms implemented by RU/compute_value.rs:70-209 plus Minus, which the
 * reference rejects (compute_value.rs:210-216) and so does this library unless the context option
 * "enable_minus" is set. Any other operator: CHQ_BINOP_OTHER.
 * CHQ_BINOP_STRING_CONCAT (`a || b`, beyond the reference; appended behind CHQ_BINOP_OTHER so that every earlier value keeps
 * its number): the bytes of `a` followed by the bytes of `b`, null if either is null; both operands must type to Utf8 (no
 * implicit cast, else CHQ_ERR_ARROW_INVALID_ARGUMENT). */
typedef enum chq_binary_operator {
  CHQ_BINOP_AND = 0, CHQ_BINOP_OR, CHQ_BINOP_PLUS, CHQ_BINOP_MINUS, CHQ_BINOP_MULTIPLY, CHQ_BINOP_DIVIDE,
  CHQ_BINOP_MODULO, CHQ_BINOP_EQ, CHQ_BINOP_NOTEQ, CHQ_BINOP_GT, CHQ_BINOP_GTEQ, CHQ_BINOP_LT, CHQ_BINOP_LTEQ,
  CHQ_BINOP_OTHER, CHQ_BINOP_STRING_CONCAT
} chq_binary_operator;

chq_expr* chq_expr_identifier(const char* name);                              /* Expr::Identifier */
chq_expr* chq_expr_compound_identifier(const char* const* parts, int n);      /* Expr::CompoundIdentifier */
chq_expr* chq_expr_number(const char* text, int is_long);                     /* Expr::Value(Value::Number(text, long)) */
chq_expr* chq_expr_boolean(int value);                                        /* Value::Boolean */
chq_expr* chq_expr_single_quoted_string(const char* bytes, int64_t len);      /* Value::SingleQuotedString */
chq_expr* chq_expr_unsupported_value(const char* debug);                      /* any other Value */
/* Expr::BinaryOp { left, op, right }; takes ownership of both children. `op_debug` is the operator's
 * Debug text, used in the BinaryOperatorNotImplemented message. */
chq_expr* chq_expr_binary_op(chq_expr* left, chq_binary_operator op, const char* op_debug, chq_expr* right);
chq_expr* chq_expr_nested(chq_expr* inner);                                   /* Expr::Nested; takes ownership */
/* Expr::Like { negated, expr, pattern, escape_char }: `operand [NOT] LIKE 'pattern' [ESCAPE 'c']`; takes ownership of
 * `operand`.  `pattern` / `pattern_len`: the bytes of the pattern when it is a single-quoted string literal (Nested around
 * it removed), NULL otherwise -- typing then returns CHQ_ERR_NOT_SUPPORTED.  `escape`: -1 for none (there is NO default
 * escape character), else one ASCII byte.  `%` = any run of bytes, `_` = one UTF-8 code point, anything else itself,
 * bytewise and case-sensitive.  The operand must type to Utf8 (else CHQ_ERR_ARROW_INVALID_ARGUMENT, as for a pattern that
 * ends in a lone escape); a compiled pattern holds at most 128 elements (literal bytes and `_`; more:
 * CHQ_ERR_NOT_SUPPORTED).  Boolean, null exactly where the operand is null. */
chq_expr* chq_expr_like(chq_expr* operand, const char* pattern, int64_t pattern_len, int negated, int escape);
/* Expr::IsNull (negated = 0) / Expr::IsNotNull (negated = 1); takes ownership of `operand`, any expression that types
 * (a bare column may have any type the library imports).  Boolean, never null. */
chq_expr* chq_expr_is_null(chq_expr* operand, int negated);
/* Expr::Function: a scalar string function `name(args)`; takes ownership of the `n_args` arguments (also when it fails and
 * returns NULL).  Names are case-insensitive.  This library's own semantics, bytewise and ASCII-only where case or
 * whitespace is involved; a CODE POINT START is a byte that is not 0x80..0xBF (what `_` takes in LIKE); invalid UTF-8 is
 * never an error and never makes a row read outside its own bytes.
 *   upper(s), lower(s)                          Utf8   bytes a..z / A..Z mapped, every other byte unchanged
 *   length(s), char_length(s),
 *   character_length(s)                         Int32  code point starts in the row
 *   octet_length(s)                             Int32  bytes in the row
 *   substring(s, p[, n]), substr(s, p[, n])     Utf8   the SQL / PostgreSQL window over 1-based code point positions: position q
 *                                                      is kept iff p <= q, q < p + n (with n) and 1 <= q <= length(s); p <= 0
 *                                                      is legal.  As bytes: from byte 0 when p <= 1, else from the p-th start
 *                                                      (or the row's end), to the max(p + n, 1)-th start (or the row's end).
 *                                                      p and n: Number literals that fit Int32 (text may carry a sign, Nested
 *                                                      allowed), else CHQ_ERR_NOT_SUPPORTED; n < 0: CHQ_ERR_ARROW_INVALID_ARGUMENT
 *   trim(s), ltrim(s), rtrim(s)                 Utf8   byte 0x20 stripped from both ends / the left / the right
 * Every result is null exactly where `s` is.  `s` must type to Utf8 (CHQ_ERR_ARROW_INVALID_ARGUMENT naming the function and
 * the type found; the same status for a wrong argument count).  A call over literals only is folded on the host with the code
 * the device runs.  A result column of more than 2^31 - 1 bytes: CHQ_ERR_ARROW_INVALID_ARGUMENT.  Any other name answers
 * exactly like chq_expr_unsupported("Function(name)").  Out of scope: trim(both 'x' from s), position / strpos, replace,
 * concat() as a function, initcap, reverse, lpad / rpad, ILIKE, implicit casts of numbers to strings, non-literal p / n,
 * LargeUtf8, and these functions as ORDER BY / GROUP BY / JOIN / PARTITION keys. */
chq_expr* chq_expr_function(const char* name, chq_expr* const* args, int n_args);
/* Expr::Case { operand, conditions, results, else_result }; takes ownership of every child, also on failure.  `operand` and
 * `else_result` may be NULL; `conditions` and `results` hold n_when >= 1 handles each.  These semantics are this library's
 * own (the reference rejects the form).
 *   Searched CASE (operand NULL): row i takes results[k] for the first k whose conditions[k] is TRUE AND VALID on that row,
 *   else else_result, else NULL.  Every condition must type to Boolean -- no implicit cast; CHQ_ERR_ARROW_INVALID_ARGUMENT
 *   names the WHEN's position and the type found.  The result type is the coercion table of the binary operators folded left
 *   to right over results[0..n), else_result: Utf8 goes only with Utf8, Boolean only with Boolean, temporal and Decimal128
 *   only with columns of the same type (the output keeps it); a pair without an entry is
 *   CHQ_ERR_UNSUPPORTED_TYPE_COERSION.  The result is null exactly where the chosen branch is, or where none is chosen and
 *   there is no ELSE; an output column is nullable iff it holds a null.  A literal branch next to columns is broadcast; a CASE
 *   over literals only is folded on the host with the rule the device runs.
 *   Simple CASE (operand given): conditions[k] is the VALUE, and WHEN k is `operand = value` by the ordinary rules and
 *   statuses of `=`; the operand is typed once.
 *   Lazy errors: a data-dependent error (integer overflow, division by zero) in results[k] counts only on rows that take
 *   it, in conditions[k] only on rows where no earlier condition was true (a NULL earlier condition is not true), in
 *   else_result only on rows where no condition was true; the first error in the order conditions, results, else_result is
 *   reported.  A literal-only sub-expression is folded at typing: `1 / 0` fails wherever it stands.
 *   More than 8 WHENs nest (WHEN 9 onward becomes a CASE in the ELSE slot).  A Utf8 result of more than 2^31 - 1 bytes:
 *   CHQ_ERR_ARROW_INVALID_ARGUMENT.
 * chq_expr_function also takes, names case-insensitive, a wrong argument count CHQ_ERR_ARROW_INVALID_ARGUMENT:
 *   coalesce(a1, .., an), n >= 1   = CASE WHEN a1 IS NOT NULL THEN a1 .. ELSE an END
 *   nullif(a, b)                   = CASE WHEN a = b THEN <null> ELSE a END, of a's own type
 * Out of scope: prefix NOT, the NULL literal, unary minus, implicit casts to Boolean in WHEN, an operator on a temporal /
 * decimal result (CHQ_ERR_NOT_SUPPORTED), LargeUtf8, and these forms as ORDER BY / GROUP BY / JOIN / PARTITION keys or
 * aggregate arguments (project first). */
chq_expr* chq_expr_case(chq_expr* operand, chq_expr* const* conditions, chq_expr* const* results, int n_when, chq_expr* else_result);
/* Expr::InList { expr, list, negated }; takes ownership of every child, also on failure.  Typing-time sugar: `expr = l1 OR
 * expr = l2 ..`, negated `expr <> l1 AND expr <> l2 ..`, with the values, nulls and statuses of that spelled-out chain; `expr`
 * is typed once.  Every item must be a literal (Nested allowed) and n must lie in 1..32, else CHQ_ERR_NOT_SUPPORTED. */
chq_expr* chq_expr_in_list(chq_expr* expr, chq_expr* const* list, int n, int negated);
/* Expr::Between { expr, negated, low, high }; takes ownership of every child, also on failure.  Typing-time sugar:
 * `expr >= low AND expr <= high`, negated `expr < low OR expr > high`, with the values, nulls and statuses of that
 * spelled-out form; `expr` is typed once. */
chq_expr* chq_expr_between(chq_expr* expr, int negated, chq_expr* low, chq_expr* high);
/* The target of chq_expr_cast.  CHQ_CAST_OTHER: any other sqlparser::ast::DataType (CHQ_ERR_NOT_SUPPORTED at typing). */
typedef enum chq_cast_type {
  CHQ_CAST_BOOLEAN = 0, CHQ_CAST_INT8, CHQ_CAST_INT16, CHQ_CAST_INT32, CHQ_CAST_INT64, CHQ_CAST_UINT8, CHQ_CAST_UINT16,
  CHQ_CAST_UINT32, CHQ_CAST_UINT64, CHQ_CAST_FLOAT16, CHQ_CAST_FLOAT32, CHQ_CAST_FLOAT64, CHQ_CAST_UTF8, CHQ_CAST_OTHER
} chq_cast_type;
/* Expr::Cast { kind: Cast | TryCast | DoubleColon, expr, data_type }: `CAST(operand AS to)`, `operand::to` (try_cast = 0) and
 * `TRY_CAST(operand AS to)` (try_cast = 1); takes ownership of `operand`, also when it fails and returns NULL.  The reference
 * rejects the form: these semantics are this library's own, modelled on arrow-cast 53 (CastOptions { safe: false } for CAST,
 * safe: true for TRY_CAST) and unpinned to it.  A null row gives a null row.  A row that FAILS below ends a CAST with
 * CHQ_ERR_ARROW_CAST (the message names the source and the target type) and becomes null under TRY_CAST.  An output column
 * is nullable iff it holds a null.  A cast to the operand's own type is the operand itself.
 *   integer -> integer        value preserved; fails iff it lies outside the target's range
 *   integer -> Float16/32/64  the exact integer rounded once, to nearest even (Float16: beyond 65504 -> +-inf); never fails
 *   float   -> integer        NaN and +-inf fail; otherwise truncated toward zero (-0.9 -> 0, also for unsigned targets;
 *                             -0.0 -> 0); fails iff the truncated value lies outside the range
 *   float   -> float          one rounding to nearest even, overflow -> +-inf, subnormals produced and consumed exactly; a
 *                             NaN keeps its sign and the top payload bits that fit, quiet bit set; never fails
 *   numeric -> Boolean        x != 0 (NaN -> true, -0.0 -> false); never fails
 *   Boolean -> numeric        1 / 0 (1.0 / 0.0); never fails
 *   Utf8    -> Boolean        the spellings of the cast under AND / OR (trimmed, case-folded t / true / y / yes / on / 1 ..);
 *                             any other string fails
 *   Utf8    -> integer        the whole row must match [+-]?[0-9]+ (`-` only for signed targets): no white space is stripped,
 *                             any number of leading zeros, `-0` is 0, and the value must fit the target; otherwise it fails
 *   integer -> Utf8           shortest decimal, `-` for negatives (1 to 20 bytes); never fails
 *   Boolean -> Utf8           `true` / `false`; never fails
 * A cast over literals only is folded on the host with the code the device runs: a failing literal CAST fails at typing
 * wherever it stands (like `1 / 0`), a failing literal TRY_CAST is a typed null.  Lazy errors: a CAST that can fail counts as
 * data-dependent for the rule of chq_expr_case, and reports failures on valid rows only.  A Utf8 result of more than
 * 2^31 - 1 bytes: CHQ_ERR_ARROW_INVALID_ARGUMENT.  CHQ_ERR_NOT_SUPPORTED: Float <-> Utf8 (a correctly rounded parse and a
 * shortest round-trip print are not built), temporal and Decimal128 operands, LargeUtf8, CHQ_CAST_OTHER. */
chq_expr* chq_expr_cast(chq_expr* operand, chq_cast_type to, int try_cast);
/* The data type of chq_expr_typed_string. */
typedef enum chq_typed_string_kind { CHQ_TYPED_STRING_DATE = 0, CHQ_TYPED_STRING_TIMESTAMP = 1 } chq_typed_string_kind;
/* Expr::TypedString { data_type, value }: `DATE '2024-03-01'`, `TIMESTAMP '2024-03-01 12:30:00.5'`.  The reference rejects the
 * form: these semantics are this library's own.
 *   DATE is YYYY-MM-DD; TIMESTAMP is YYYY-MM-DD, a space or `T`, HH:MM[:SS[.f{1,9}]].  Years 0001 - 9999, a day of the proleptic
 *   Gregorian calendar, hours 00 - 23, minutes and seconds 00 - 59, no zone suffix, no white space around it; anything else is
 *   CHQ_ERR_ARROW_CAST at typing, the message quoting the literal.
 *   The literal has no Arrow type of its own.  It stands beside a Date32 / Date64 / Timestamp operand of a comparison (either
 *   order; BETWEEN and IN lists are comparisons) and takes that operand's DataType: a DATE is days beside Date32, milliseconds
 *   beside Date64, midnight in the unit beside Timestamp(unit); a TIMESTAMP is admitted beside Timestamp(unit) only
 *   (CHQ_ERR_NOT_SUPPORTED beside a Date).  A Timestamp with a time zone is admitted for `UTC` and `+00:00`, the literal is then
 *   UTC; any other zone is CHQ_ERR_NOT_SUPPORTED (there is no zone database).  Fraction digits finer than the unit, and a value
 *   that does not fit the unit's Int64 (`TIMESTAMP '2300-01-01 00:00:00'` beside nanoseconds), are CHQ_ERR_ARROW_CAST.  The
 *   comparison then is the integer comparison of the raw values.
 *   Beside a non-temporal operand: CHQ_ERR_UNSUPPORTED_TYPE_COERSION, as for `date_column < 5`.  Alone, beside another literal,
 *   under any other operator, as a function argument or CASE branch, beside Time32 / Time64 / Duration / Decimal128:
 *   CHQ_ERR_NOT_SUPPORTED.
 * The temporal functions come through chq_expr_function, names and fields case-insensitive:
 *   date_part('field', e) -> Int32   what EXTRACT(field FROM e) is sent as.  field: year, quarter, month, week (ISO 8601), day,
 *                                    doy, dow (Sunday = 0), hour, minute, second (whole seconds)
 *   date_trunc('unit', e)            of e's own DataType (unit and zone kept).  unit: year, quarter, month, week (Monday), day,
 *                                    hour, minute, second; on Date32 the units below day are the identity
 *   e is a Date32 / Date64 (read as milliseconds) / Timestamp (no zone, `UTC`, `+00:00`) column or a date_trunc of one;
 *   date_part also takes Time32 / Time64 columns, for hour / minute / second.  The value is split by FLOOR division into days
 *   since 1970-01-01 and a time of day (-1 s is 1969-12-31 23:59:59); the calendar is the proleptic Gregorian one.  No row
 *   fails: a row whose date lies outside years -262143 .. 262142, a Time outside one day, and a truncation that does not fit the
 *   raw integer come out null.  Statuses: a field / unit that is not a string literal or not in the list, and any other zone,
 *   CHQ_ERR_NOT_SUPPORTED; any other operand type, and a date field of a Time, CHQ_ERR_ARROW_INVALID_ARGUMENT.  A date_trunc
 *   result compares with a literal or a value of the same DataType; chq_ctx_last_stats counts the launches and bytes. */
chq_expr* chq_expr_typed_string(chq_typed_string_kind kind, const char* bytes, int64_t len);
chq_expr* chq_expr_unsupported(const char* debug);                            /* any other Expr variant */
void chq_expr_free(chq_expr* e);

/* sqlparser::ast::SelectItem, RU/record_projection.rs:25-69 */
typedef enum chq_select_item_kind {
  CHQ_ITEM_WILDCARD = 0, CHQ_ITEM_QUALIFIED_WILDCARD, CHQ_ITEM_UNNAMED_EXPR, CHQ_ITEM_EXPR_WITH_ALIAS
} chq_select_item_kind;
typedef struct chq_select_item {
  int kind;               /* chq_select_item_kind */
  const chq_expr* expr;   /* UNNAMED_EXPR / EXPR_WITH_ALIAS */
  const char* alias;      /* EXPR_WITH_ALIAS */
} chq_select_item;

/* table_aliases: &Vec<Vec<String>> -- one alias list per column (RU/record_aliases.rs:12-59).
 * `n_columns` may be smaller than the batch's column count (the reference's tests pass vec![]). */
typedef struct chq_alias_list { const char* const* aliases; int n; } chq_alias_list;
typedef struct chq_table_aliases { const chq_alias_list* columns; int n_columns; } chq_table_aliases;

/* ---- the path -------------------------------------------------------------------------------- */
/* `out_device`: ARROW_DEVICE_CPU or ARROW_DEVICE_ROCM. On success *out / *out_schema are filled and
 * must be released by the caller; on failure they are left released (release == NULL). */

/* RU/filter_record.rs:21-39: evaluate `expr` to a BooleanArray, keep the rows where it is true and
 * valid, every column, original order, same schema; possibly zero rows. */
chq_status chq_filter_record(chq_ctx* ctx, const struct ArrowDeviceArray* rec, const struct ArrowSchema* schema,
                             const chq_table_aliases* table_aliases, const chq_expr* expr, int out_device,
                             struct ArrowDeviceArray* out, struct ArrowSchema* out_schema);

/* chq_filter_record over `n_records` batches of ONE schema, in one call: out[i] is exactly what
 * chq_filter_record(recs[i]) returns, and on failure the status / message are those of the first
 * batch (in array order) whose single call fails; nothing is returned then.  This is the loop of
 * filter_task.rs:78-126 (get_next_record -> filter_record -> send) hoisted below the boundary: the
 * reference's batches are 10 000 rows (src/planner/physical_planner.rs:323), far too small to fill
 * the GPU one at a time.  When every column is fixed-width without nulls, all batches run in ONE
 * kernel launch (one chained compaction; out[i] are slices of one dense buffer per column); other
 * groups are processed batch by batch inside the call.  `outs` / `out_schemas`: n_records entries. */
chq_status chq_filter_records(chq_ctx* ctx, int n_records, const struct ArrowDeviceArray* const* recs,
                              const struct ArrowSchema* schema, const chq_table_aliases* table_aliases,
                              const chq_expr* expr, int out_device, struct ArrowDeviceArray* outs,
                              struct ArrowSchema* out_schemas);

/* The same call with the results joined: ONE output batch = the surviving rows of recs[0], recs[1], ... back to
 * back (input order), and rows_per_record[i] (optional, n_records entries) = how many of them came from recs[i].
 * This is the batch coalescing the reference plans for its exchange (DEV_NOTES.md:175-182):
 * downstream operators see one large batch instead of 10^5 small ones; a caller that needs the per-record ids back
 * slices the output at the running sums of rows_per_record.  In the one-launch case the output IS the kernel's dense
 * buffer, so nothing is copied or exported per input batch. */
chq_status chq_filter_records_coalesced(chq_ctx* ctx, int n_records, const struct ArrowDeviceArray* const* recs,
                                        const struct ArrowSchema* schema, const chq_table_aliases* table_aliases,
                                        const chq_expr* expr, int out_device, struct ArrowDeviceArray* out,
                                        struct ArrowSchema* out_schema, int64_t* rows_per_record);

/* RU/record_projection.rs:16-76 */
chq_status chq_project_record(chq_ctx* ctx, const chq_select_item* fields, int n_fields,
                              const struct ArrowDeviceArray* rec, const struct ArrowSchema* schema,
                              const chq_table_aliases* table_aliases, int out_device,
                              struct ArrowDeviceArray* out, struct ArrowSchema* out_schema);

/* RU/compute_value.rs:57-344: returns ArrayDatum { array, is_scalar } */
chq_status chq_compute_value(chq_ctx* ctx, const struct ArrowDeviceArray* rec, const struct ArrowSchema* schema,
                             const chq_table_aliases* table_aliases, const chq_expr* expr, int out_device,
                             struct ArrowDeviceArray* out, struct ArrowSchema* out_schema, int* out_is_scalar);

/* filter_record followed by project_record on the surviving rows -- the reference's
 * filter -> exchange -> materialize sequence (filter_task.rs:99, materialize_files_task.rs:110) fused
 * into one call so the filtered batch never leaves the GPU. */
chq_status chq_filter_project_record(chq_ctx* ctx, const chq_expr* predicate, const chq_select_item* fields,
                                     int n_fields, const struct ArrowDeviceArray* rec,
                                     const struct ArrowSchema* schema, const chq_table_aliases* table_aliases,
                                     int out_device, struct ArrowDeviceArray* out, struct ArrowSchema* out_schema);

/* ---- host half only (no GPU, no context) --------------------------------------------------------- */
/* Types `expr` against `schema` (a struct schema as in the record calls) exactly as chq_compute_value would --
 * literal typing, column / alias lookup, the coercion table, constant folding, the arrow length rules -- and writes
 * a description into `buf`: "result <Type> scalar=<0|1> len1=<0|1>", then the folded value, the column index or the
 * listing of the device program.  Returns the static status the record calls would return for a batch of n_rows rows
 * (message in `buf`).  Used by the CPU test tier and for debugging planners; touches no device. */
chq_status chq_plan_describe(const struct ArrowSchema* schema, const chq_table_aliases* table_aliases,
                             const chq_expr* expr, int64_t n_rows, int enable_minus, char* buf, size_t buf_len);

/* ---- device residency helpers ----------------------------------------------------------------- */
/* Copy a host batch into HBM / a device batch back to host memory. */
chq_status chq_record_to_device(chq_ctx* ctx, const struct ArrowDeviceArray* rec, const struct ArrowSchema* schema,
                                struct ArrowDeviceArray* out, struct ArrowSchema* out_schema);
chq_status chq_record_to_host(chq_ctx* ctx, const struct ArrowDeviceArray* rec, const struct ArrowSchema* schema,
                              struct ArrowDeviceArray* out, struct ArrowSchema* out_schema);

/* The data-plane half of the exchange step, GPU to GPU: copy a batch that lives in the HBM of `src_ctx`'s device into
 * the HBM of `dst_ctx`'s device with hipMemcpyPeerAsync -- peer to peer over the xGMI link of the pair, no host staging,
 * no collective.  This is what moves a record when the DAG puts its consumer on another GPU (one filter instance per
 * GPU feeding one materialize instance) for a worker that runs several operator instances in ONE process
 * (src/worker/query_worker.rs:35-39), one chq_ctx per GPU.  The reference's exchange semantics are the caller's and do
 * not change: the record keeps its record_id and table_aliases, the inbound exchange is acked only after the copy was
 * handed over (exchange_operator.rs:621-667, requests/send_record_request.rs:33-104).
 * The copies are enqueued on dst_ctx's stream; the call returns without waiting for them.  out->sync_event points to a
 * hipEvent_t (owned by `out`, destroyed by its release callback) recorded behind the last copy: every chq call that takes
 * `out` as input waits on it, any other consumer must (Arrow C Device Data Interface).  `rec` must stay alive until that
 * event has completed.  src_ctx == dst_ctx's device is allowed (a device-local deep copy). */
chq_status chq_record_copy_to_peer(chq_ctx* src_ctx, chq_ctx* dst_ctx, const struct ArrowDeviceArray* rec,
                                   const struct ArrowSchema* schema, struct ArrowDeviceArray* out,
                                   struct ArrowSchema* out_schema);

/* ---- Arrow IPC with the message body in HBM ------------------------------------------------------------------------ */
/* The wire format the reference puts a batch in when it leaves the process: an Arrow IPC *stream* -- Schema message,
 * one RecordBatch message, end-of-stream -- written by arrow::ipc::writer::StreamWriter and read back by
 * arrow::ipc::reader::StreamReader (src/handlers/message_handler/messages/exchange.rs:145-197, 247-276).  For a batch
 * that lives on the GPU the two metadata flatbuffers are built on the host and the message BODY (every Arrow buffer,
 * rebased to offset 0, 64-byte aligned, back to back) is assembled in ONE HBM allocation, so it travels with a single
 * RCCL send / peer copy, or one D2H copy when it must cross TCP.  The bytes
 *     header[0 .. header_len)  ++  body[0 .. body_len)  ++  end_of_stream[0 .. 8)
 * are exactly the stream an Arrow reader expects.  Dictionaries, compression and nested types: CHQ_ERR_NOT_SUPPORTED. */
typedef struct chq_ipc_message {
  const uint8_t* header;      /* host memory: Schema message + framing and metadata of the RecordBatch message */
  int64_t header_len;
  const void* body;           /* HBM (ARROW_DEVICE_ROCM) or host memory (ARROW_DEVICE_CPU), see body_device_type */
  int64_t body_len;
  int32_t body_device_type;
  int32_t body_device_id;
  uint8_t end_of_stream[8];   /* 0xFFFFFFFF 0x00000000 */
  void (*release)(struct chq_ipc_message*);
  void* private_data;
} chq_ipc_message;

/* `rec`: host or device resident.  `body_device`: ARROW_DEVICE_ROCM (the body stays in HBM) or ARROW_DEVICE_CPU. */
chq_status chq_record_to_ipc(chq_ctx* ctx, const struct ArrowDeviceArray* rec, const struct ArrowSchema* schema,
                             int body_device, chq_ipc_message* out);
/* Inverse.  `stream` (host memory) holds the Schema message and the RecordBatch message's metadata; the body is `body`
 * (in memory of kind `body_device_type`), or -- when `body` is NULL -- follows the metadata inside `stream` itself, i.e.
 * `stream` is a complete Arrow IPC stream as any Arrow writer produces it.  The body is moved to `out_device` with one
 * copy; the returned batch owns it. */
chq_status chq_record_from_ipc(chq_ctx* ctx, const uint8_t* stream, int64_t stream_len, const void* body, int64_t body_len,
                               int body_device_type, int out_device, struct ArrowDeviceArray* out,
                               struct ArrowSchema* out_schema);

/* Host half only (no GPU, no context): what the metadata of an Arrow IPC stream says -- "rows R body B body_at P", one
 * "field <name> <format> nullable=<0|1> nulls=<k>" line per column, one "buffer <offset> <length>" line per buffer.  Used
 * by the CPU test tier (the flatbuffer reader against pyarrow's writer) and for debugging. */
chq_status chq_ipc_describe(const uint8_t* stream, int64_t stream_len, char* buf, size_t buf_len);

/* ---- Parquet scan with the page decode on the GPU --------------------------------------------
 * Replaces the decode the reference does with the `parquet` crate in front of the filter path
 * (operators/table_func_tasks/read_files_task.rs:233-282: ParquetRecordBatchStreamBuilder::new(reader) ...
 * with_batch_size(max_rows_per_batch)): the caller hands over the file's bytes (host memory, borrowed until
 * chq_parquet_close), the library parses footer and page headers on the host, uploads each column chunk as it lies in the
 * file and decodes the pages into Arrow buffers in HBM.  One call yields one ROW GROUP as one device-resident batch (the
 * reference cuts 10 000-row batches; slices of the result are zero-copy, and the filter kernels prefer large batches).
 * Scope: flat schemas; BOOLEAN, INT32, INT64, FLOAT, DOUBLE, BYTE_ARRAY annotated String; required / optional columns;
 * PLAIN and RLE_DICTIONARY / PLAIN_DICTIONARY (also mixed inside a chunk: the writers' dictionary fallback); data pages
 * V1 and V2; UNCOMPRESSED (what the reference's writers produce: create_sample_data.rs:222,
 * materialize_files_task.rs:128-133) and SNAPPY (what pyarrow / Spark / DuckDB write by default; the pages are inflated on
 * the GPU).  Everything else (GZIP, ZSTD, LZ4, BROTLI pages; nested schemas; DELTA_* encodings): CHQ_ERR_NOT_SUPPORTED, the
 * message names the feature. */
typedef struct chq_parquet chq_parquet;
/* Footer + page headers; no GPU, no context.  On failure *out is NULL and `err` (if given) receives the message. */
chq_status chq_parquet_open(const uint8_t* file, int64_t file_len, chq_parquet** out, char* err, size_t err_len);
/* The same over a RANGE READER instead of the whole file in memory: the reference reads Parquet through opendal ranges
 * (read_files_task.rs:233-250: op.reader_with(path), ParquetRecordBatchStreamBuilder over it), i.e. the footer and then only
 * the column chunks a query decodes.  `read(user, offset, length, dst)` must fill dst[0 .. length) with the file's bytes
 * [offset, offset + length) and return 0; any other value fails the call.  Open reads the file's tail (footer) and nothing
 * else; every read call then fetches exactly the column chunks it decodes, one `read` per chunk, from the calling thread.
 * `read` / `user` must stay valid until chq_parquet_close. */
typedef int (*chq_read_range_fn)(void* user, int64_t offset, int64_t length, uint8_t* dst);
chq_status chq_parquet_open_reader(int64_t file_len, chq_read_range_fn read, void* user, chq_parquet** out, char* err, size_t err_len);
void chq_parquet_close(chq_parquet* pq);
int32_t chq_parquet_num_columns(const chq_parquet* pq);
/* Name of column `column` (valid until chq_parquet_close), or NULL. */
const char* chq_parquet_column_name(const chq_parquet* pq, int32_t column);
int32_t chq_parquet_num_row_groups(const chq_parquet* pq);
int64_t chq_parquet_row_group_num_rows(const chq_parquet* pq, int32_t row_group);
/* "rows R row_groups G columns C" / "column <name> <physical> <required|optional> [utf8]" / "rg <i> rows <n>" /
 * "chunk <col> values <n> codec <c> pages <p>" / "page <type> values <n> enc <e> bytes <b> header <h>" lines (CPU test tier) */
chq_status chq_parquet_describe(const chq_parquet* pq, char* buf, size_t buf_len);
/* Decode one row group.  `out_device`: ARROW_DEVICE_ROCM (stays in HBM) or ARROW_DEVICE_CPU (copied down). */
chq_status chq_parquet_read_row_group(chq_ctx* ctx, const chq_parquet* pq, int32_t row_group, int out_device,
                                      struct ArrowDeviceArray* out, struct ArrowSchema* out_schema);
/* Row groups [first, first + count), one batch each in outs[i] / out_schemas[i]: all of them are in flight together (the
 * upload of one overlaps the decode of the others) and the host synchronises twice per call instead of twice per row
 * group.  On failure nothing is returned. */
chq_status chq_parquet_read_row_groups(chq_ctx* ctx, const chq_parquet* pq, int32_t first, int32_t count, int out_device,
                                       struct ArrowDeviceArray* outs, struct ArrowSchema* out_schemas);

/* Column pruning (the reference's own TODO, DEV_NOTES.md:123): the same call for the `n_columns` columns listed in
 * `columns` (indices into the file's schema, in the order the output batch should carry them; NULL = every column).  Only
 * those columns' chunks are fetched (range reader), uploaded and decoded.  chq_ctx_last_stats afterwards: rows_in = rows
 * decoded, bytes_read_alg = file bytes sent to the GPU, bytes_written_alg = Arrow bytes produced. */
chq_status chq_parquet_read_columns(chq_ctx* ctx, const chq_parquet* pq, int32_t first, int32_t count, const int32_t* columns,
                                    int32_t n_columns, int out_device, struct ArrowDeviceArray* outs, struct ArrowSchema* out_schemas);

/* ---- Parquet write with the page encode on the GPU ---------------------------------------
 * Replaces the encode the reference does with the `parquet` crate behind project_record
 * (operators/materialize_tasks/materialize_files_task.rs:128-141: AsyncArrowWriter::try_new(writer, schema, None),
 * write(&rec), close() -- one file with one row group per record).  `rec` (host or device resident) becomes one complete
 * Parquet file image in host memory, ready for the storage writer: the value streams of the pages are produced in HBM and
 * copied once into place, headers and footer are written on the host.  Format: PLAIN, UNCOMPRESSED, data pages V1 of
 * "parquet_page_rows" rows, definition levels = the Arrow validity bitmap, chunk statistics (null_count, min / max).  Every
 * Parquet reader decodes it; it is not byte-identical to the parquet crate's output (which dictionary-encodes first and
 * adds page indexes).
 * Types: Int32, Int64, Float32, Float64, Boolean, Utf8; others CHQ_ERR_NOT_SUPPORTED. */
typedef struct chq_parquet_image {
  const uint8_t* data;   /* host memory, `len` bytes: "PAR1" ... footer ... "PAR1" */
  int64_t len;
  void (*release)(struct chq_parquet_image*);
  void* private_data;
} chq_parquet_image;
chq_status chq_record_to_parquet(chq_ctx* ctx, const struct ArrowDeviceArray* rec, const struct ArrowSchema* schema,
                                 chq_parquet_image* out);
/* The same for `n_records` batches of ONE schema (names, types and nullability must agree: CHQ_ERR_ARROW_INVALID_ARGUMENT
 * otherwise): one file, one row group per batch, in order -- the compaction of several records into a larger file that the
 * reference's DEV_NOTES.md:117-121 plans for the materialize task. */
chq_status chq_records_to_parquet(chq_ctx* ctx, int n_records, const struct ArrowDeviceArray* const* recs,
                                  const struct ArrowSchema* schema, chq_parquet_image* out);

/* ---- ORDER BY: stable multi-key sort of a record batch --------------------------------------------
 * The reference has no ORDER BY yet; these semantics are this library's (arrow-rs lexsort_to_indices with explicit
 * SortOptions):
 *   - a key is a column (Identifier / CompoundIdentifier), resolved through `table_aliases` like compute_value resolves
 *     them (a missing column: the same status); any other expression: CHQ_ERR_NOT_SUPPORTED.
 *   - key types: Int8..64, UInt8..64, Float16/32/64, Boolean (false < true), Date32/64, Time32/64, Timestamp and Duration
 *     (as their signed integers), Decimal128 (signed 128-bit), Utf8 (bytewise, a proper prefix first).  Floats follow
 *     totalOrder: -NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN.  Other types (FixedSizeBinary, ...): CHQ_ERR_NOT_SUPPORTED.
 *   - `descending` reverses the value order; `nulls_first` puts null keys before (else after) the others, whatever the
 *     direction.  Both are explicit here (the SQL defaults, ASC and NULLS LAST for ASC / NULLS FIRST for DESC, are the
 *     front-end's).
 *   - stable: rows with equal keys keep input order (for a group: batch order, then row order).
 *   - every column comes out permuted; the schema is the input's; null counts are exact; output conventions are those of
 *     chq_filter_record.  `limit` -1: every row, else the first min(limit, rows) rows of the sorted order.
 *   - fewer than 2^32 rows per call (else CHQ_ERR_NOT_SUPPORTED); an output Utf8 column past int32 offsets:
 *     CHQ_ERR_ARROW_INVALID_ARGUMENT naming it.
 * Inputs may be host or device resident and sliced; `out_device` is ARROW_DEVICE_CPU or ARROW_DEVICE_ROCM.  On failure
 * nothing is returned (release == NULL). */
typedef struct chq_sort_key {
  const chq_expr* column;
  int descending;
  int nulls_first;
} chq_sort_key;
chq_status chq_sort_record(chq_ctx* ctx, const struct ArrowDeviceArray* rec, const struct ArrowSchema* schema,
                           const chq_table_aliases* table_aliases, const chq_sort_key* keys, int n_keys, int64_t limit,
                           int out_device, struct ArrowDeviceArray* out, struct ArrowSchema* out_schema);
/* The same over `n_records` batches of ONE schema: ONE joined, sorted batch (the group is joined on the device first). */
chq_status chq_sort_records(chq_ctx* ctx, int n_records, const struct ArrowDeviceArray* const* recs,
                            const struct ArrowSchema* schema, const chq_table_aliases* table_aliases,
                            const chq_sort_key* keys, int n_keys, int64_t limit, int out_device,
                            struct ArrowDeviceArray* out, struct ArrowSchema* out_schema);

/* ---- GROUP BY: grouped COUNT / SUM / MIN / MAX / AVG / COUNT(DISTINCT) on top of the stable sort -----
 * The reference has no GROUP BY; these semantics are this library's own (unpinned), chosen so that none of them depends on
 * the order in which rows are combined:
 *   - zero or more keys, each a column (Identifier / CompoundIdentifier) resolved exactly like a sort key (a missing
 *     column: the evaluator's status; any other expression: CHQ_ERR_NOT_SUPPORTED); the key types are those of ORDER BY.
 *   - two rows are in one group iff for every key both values are null, or both are non-null with EQUAL BIT PATTERNS: for
 *     floats that is totalOrder equality (-0 and +0 are two groups, so are NaNs with different payloads), for Utf8 equal
 *     length and equal bytes.  Null is a group of its own.  No key: one group over all rows, which exists even for zero
 *     rows (COUNT 0, every other aggregate null).  At least one key and zero rows: zero output rows.
 *   - one output row per group, in a guaranteed order: ascending by the keys in the order given, nulls last.
 *   - one output column per item, in item order, named `name`:
 *       CHQ_AGG_KEY         key `key_index`: the input field's type and nullability, the value of the group's first row in
 *                           input order (for a group of batches: batch order, then row order)
 *       CHQ_AGG_COUNT_STAR  rows of the group; CHQ_AGG_COUNT: non-null values of `column`.  Int64, not nullable.
 *       CHQ_AGG_SUM         nulls skipped; Int8..64 -> Int64, UInt8..64 -> UInt64, Float32/64 -> Float64; nullable, null for
 *                           a group without a non-null value.  Integer overflow is decided on the EXACT total of the group,
 *                           never on an intermediate ({INT64_MAX, 1, -5} is INT64_MAX - 4); a total outside the result type
 *                           fails the whole call with CHQ_ERR_ARROW_ARITHMETIC_OVERFLOW naming the output column.  Float
 *                           sums are IEEE binary64 additions (Float32 widens exactly; NaN and +-inf propagate, +inf with
 *                           -inf is NaN) combined in an order fixed by the input: bit-identical from run to run.
 *       CHQ_AGG_MIN / MAX   nulls skipped; the input type, nullable; Int8..64, UInt8..64, Float16/32/64 in totalOrder, and
 *                           Date, Time, Timestamp, Duration and decimals of up to 8 bytes as signed integers.  The result
 *                           is the bits of an actual input value.
 *       CHQ_AGG_AVG         nulls skipped; the input types of SUM; Float64, nullable, null for a group without a non-null
 *                           value.  Floats: the group's SUM -- the very bits a CHQ_AGG_SUM item over the same column in the
 *                           same call gives -- divided by binary64(count) in one IEEE division (NaN and +-inf propagate).
 *                           Integers: RN(T) / binary64(count), T the EXACT 128-bit total of the group and RN its rounding to
 *                           the nearest binary64, ties to even (Python: float(T) / float(count)).  AVG never fails with
 *                           CHQ_ERR_ARROW_ARITHMETIC_OVERFLOW: the average of {INT64_MAX, INT64_MAX} is 9.223372036854775807e18.
 *       CHQ_AGG_COUNT_DISTINCT  distinct non-null values of `column` in the group, equal by BIT PATTERN as the keys are (-0
 *                           and +0 are two values, so are NaNs with different payloads; Utf8: length and bytes).  Int64, not
 *                           nullable; 0 for a group whose values are all null and for the group over zero rows.  `column` may
 *                           have any type ORDER BY takes as a key.  Cost: one more sort (by the keys, then `column`) and one
 *                           more run finding per distinct argument column of the call, shared by the items that name it.
 *     CHQ_ERR_NOT_SUPPORTED, naming the column and its type: SUM and AVG over Float16, Boolean, temporal types, decimals,
 *     Utf8; MIN / MAX over Utf8, Boolean, Decimal128; COUNT_DISTINCT over a type without an order.  A kind outside 0..7:
 *     CHQ_ERR_ARROW_INVALID_ARGUMENT.  An empty item list, or a key_index outside the keys:
 *     CHQ_ERR_ARROW_INVALID_ARGUMENT.
 *   - fewer than 2^32 rows per call (else CHQ_ERR_NOT_SUPPORTED).
 * HAVING (the Python front-end composes it from this call and chq_filter_record), VAR / STDDEV, SUM(DISTINCT), expressions
 * as keys or arguments, and partial / merge aggregation across instances are
 * out of scope (the route to several instances is chq_partition_records by the keys: a group lies wholly inside one partition).  Inputs may be host or device resident and sliced; `out_device` is ARROW_DEVICE_CPU or ARROW_DEVICE_ROCM.
 * On failure nothing is returned (release == NULL). */
typedef enum chq_agg_kind {
  CHQ_AGG_KEY = 0,
  CHQ_AGG_COUNT_STAR = 1,
  CHQ_AGG_COUNT = 2,
  CHQ_AGG_SUM = 3,
  CHQ_AGG_MIN = 4,
  CHQ_AGG_MAX = 5,
  CHQ_AGG_AVG = 6,
  CHQ_AGG_COUNT_DISTINCT = 7
} chq_agg_kind;
typedef struct chq_agg_item {
  int kind;                /* chq_agg_kind */
  int key_index;           /* CHQ_AGG_KEY: index into `keys` */
  const chq_expr* column;  /* COUNT, SUM, MIN, MAX, AVG, COUNT_DISTINCT: the argument column; NULL otherwise */
  const char* name;        /* output column name */
} chq_agg_item;
chq_status chq_aggregate_record(chq_ctx* ctx, const struct ArrowDeviceArray* rec, const struct ArrowSchema* schema,
                                const chq_table_aliases* table_aliases, const chq_expr* const* keys, int n_keys,
                                const chq_agg_item* items, int n_items, int out_device, struct ArrowDeviceArray* out,
                                struct ArrowSchema* out_schema);
/* The same over `n_records` batches of ONE schema, as if they were one batch (the group is joined on the device first). */
chq_status chq_aggregate_records(chq_ctx* ctx, int n_records, const struct ArrowDeviceArray* const* recs,
                                 const struct ArrowSchema* schema, const chq_table_aliases* table_aliases,
                                 const chq_expr* const* keys, int n_keys, const chq_agg_item* items, int n_items,
                                 int out_device, struct ArrowDeviceArray* out, struct ArrowSchema* out_schema);

/* ---- Window functions: fn(...) OVER (PARTITION BY ... ORDER BY ...) -----------------------------
 * The reference has no window functions; these semantics are this library's own (unpinned).  One call takes a group of
 * n >= 1 batches of one schema (host or device resident, sliced or empty; joined on the device first, as chq_sort_records
 * does), zero or more PARTITION BY keys, zero or more ORDER BY keys (chq_sort_key: each with `descending` / `nulls_first`)
 * and one or more items, and returns EVERY INPUT ROW IN INPUT ORDER (batch order, then row order) with one more column
 * per item:
 *   - keys are columns (Identifier / CompoundIdentifier) resolved exactly like a sort key (a missing column: the
 *     evaluator's status; any other expression: CHQ_ERR_NOT_SUPPORTED); the key types are those of ORDER BY, any other
 *     type: CHQ_ERR_NOT_SUPPORTED naming the column and its Arrow type.
 *   - the rows are ordered by the partition keys (ascending, nulls last; the order AMONG partitions cannot be observed),
 *     then by the order keys with their flags; the order is stable, ties keep input order.
 *   - two rows are in one PARTITION iff for every partition key both values are null, or both are non-null with EQUAL BIT
 *     PATTERNS (GROUP BY's rule: -0 and +0 differ, so do NaNs with different payloads; Utf8: length, then bytes).  No
 *     partition key: one partition.  Two rows of a partition are PEERS iff the same holds for every order key; no order
 *     key: the whole partition is one peer group.
 *   - output: ONE batch.  First every input column (same fields, same values, exact null counts), then one column per
 *     item, in item order, named `name`.  Zero rows in: zero rows out with the full schema.
 *   - items, by `kind`:
 *       CHQ_WIN_ROW_NUMBER / RANK / DENSE_RANK   Int64, not nullable, 1-based inside the partition: the row's sorted position;
 *                            the row number of its first peer; the number of peer groups up to and including its own.
 *       CHQ_WIN_LAG / LEAD   the value of `column` in the row `offset` (>= 0) sorted positions before / behind inside the
 *                            partition, null where there is none (no default-value argument); offset 0: the row's own
 *                            value; a negative offset: CHQ_ERR_ARROW_INVALID_ARGUMENT.  Every column type is accepted (Utf8,
 *                            Boolean, Decimal128, ...); the output field has the input's type and is nullable.
 *       CHQ_WIN_COUNT_STAR / COUNT / SUM / MIN / MAX   input types, result types, null skipping and the
 *                            CHQ_ERR_NOT_SUPPORTED cases are EXACTLY those of chq_aggregate_records, evaluated over `frame`:
 *                              CHQ_FRAME_PARTITION          the whole partition
 *                              CHQ_FRAME_ROWS_TO_CURRENT    the partition's first row through this row
 *                              CHQ_FRAME_RANGE_TO_CURRENT   the partition's first row through this row's LAST PEER (SQL's
 *                                                           default when ORDER BY is written)
 *                            COUNTs are Int64, not nullable; SUM / MIN / MAX are nullable and null where the frame holds no
 *                            non-null value.  Integer SUM accumulates in 128 bits; if the exact total of ANY ROW'S FRAME is
 *                            outside the result type the whole call fails with CHQ_ERR_ARROW_ARITHMETIC_OVERFLOW naming the
 *                            output column ({INT64_MAX, 1, -5} in that sorted order succeeds under PARTITION and fails under
 *                            ROWS_TO_CURRENT).  Float SUM: IEEE binary64 additions (Float32 widens exactly; NaN and +-inf
 *                            propagate) combined in an order fixed by the sorted positions alone: bit-identical from run to
 *                            run, and all rows of one peer group under RANGE, all rows of one partition under PARTITION,
 *                            carry the same bits.
 *     `frame` is ignored for the ranking kinds and LAG / LEAD.  An empty item list, an unknown kind or frame, or a missing
 *     `column` where one is needed: CHQ_ERR_ARROW_INVALID_ARGUMENT.
 *   - fewer than 2^32 rows per call (else CHQ_ERR_NOT_SUPPORTED).  `out_device` is ARROW_DEVICE_CPU or ARROW_DEVICE_ROCM.
 *     On failure nothing is returned (release == NULL).  chq_ctx_last_stats: rows_in = rows_out = the rows of the group.
 * Out of scope: bounded frames (n PRECEDING / FOLLOWING), FIRST_VALUE / LAST_VALUE / NTILE, AVG, expressions as keys or
 * arguments, several window specifications in one call, and multi-instance execution (the route is chq_partition_records by
 * the PARTITION BY keys: a partition lies wholly inside one hash partition). */
typedef enum chq_window_kind {
  CHQ_WIN_ROW_NUMBER = 0,
  CHQ_WIN_RANK = 1,
  CHQ_WIN_DENSE_RANK = 2,
  CHQ_WIN_LAG = 3,
  CHQ_WIN_LEAD = 4,
  CHQ_WIN_COUNT_STAR = 5,
  CHQ_WIN_COUNT = 6,
  CHQ_WIN_SUM = 7,
  CHQ_WIN_MIN = 8,
  CHQ_WIN_MAX = 9
} chq_window_kind;
typedef enum chq_window_frame {
  CHQ_FRAME_PARTITION = 0,
  CHQ_FRAME_ROWS_TO_CURRENT = 1,
  CHQ_FRAME_RANGE_TO_CURRENT = 2
} chq_window_frame;
typedef struct chq_window_item {
  int kind;                /* chq_window_kind */
  int frame;               /* chq_window_frame: the aggregates */
  int64_t offset;          /* LAG, LEAD */
  const chq_expr* column;  /* LAG, LEAD, COUNT, SUM, MIN, MAX: the argument column; NULL otherwise */
  const char* name;        /* output column name */
} chq_window_item;
chq_status chq_window_record(chq_ctx* ctx, const struct ArrowDeviceArray* rec, const struct ArrowSchema* schema,
                             const chq_table_aliases* table_aliases, const chq_expr* const* partition_by, int n_partition_by,
                             const chq_sort_key* order_by, int n_order_by, const chq_window_item* items, int n_items,
                             int out_device, struct ArrowDeviceArray* out, struct ArrowSchema* out_schema);
/* The same over `n_records` batches of ONE schema, as if they were one batch (the group is joined on the device first). */
chq_status chq_window_records(chq_ctx* ctx, int n_records, const struct ArrowDeviceArray* const* recs,
                              const struct ArrowSchema* schema, const chq_table_aliases* table_aliases,
                              const chq_expr* const* partition_by, int n_partition_by, const chq_sort_key* order_by,
                              int n_order_by, const chq_window_item* items, int n_items, int out_device,
                              struct ArrowDeviceArray* out, struct ArrowSchema* out_schema);

/* ---- JOIN: sort-merge equi-join of two groups of record batches -----------------------------------
 * The reference has no join; the semantics of INNER are derived from what it has: THE RESULT IS EXACTLY WHAT THE
 * REFERENCE'S filter_record RETURNS ON THE CROSS PRODUCT OF THE TWO INPUTS, LEFT-MAJOR, UNDER
 * `l.k0 = r.k0 AND l.k1 = r.k1 ...` (whenever the two sides of every key have one type).  The other kinds are defined on
 * top of INNER.  For every kind:
 *   - keys: one or more (left column, right column) pairs, each side a column (Identifier / CompoundIdentifier) resolved
 *     against its own side's schema and table aliases exactly like a sort key (a missing column: the evaluator's status; any
 *     other expression: CHQ_ERR_NOT_SUPPORTED).  No key: CHQ_ERR_ARROW_INVALID_ARGUMENT -- there is no cross join.
 *   - key types: those of ORDER BY, and the two columns of a pair must have the IDENTICAL Arrow C format string (the rule
 *     the comparisons of temporal and decimal types follow).  Different types (Int32 with Int64, ...): CHQ_ERR_NOT_SUPPORTED
 *     naming both columns and both types, the caller's left first -- the reference would coerce, this build does not.
 *     FixedSizeBinary and other types without an order: CHQ_ERR_NOT_SUPPORTED.
 *   - equality: two non-null values are equal iff their BIT PATTERNS are equal: for floats totalOrder equality (-0 and +0
 *     differ, NaNs are equal iff their payloads are), for Utf8 equal length and equal bytes, likewise Boolean and Decimal128.
 *     A NULL KEY NEVER MATCHES ANYTHING, a null included (`=` yields null and the filter drops the row).
 *   - inputs: each side a group of n >= 1 batches of one schema, host or device resident, sliced or empty; each side is
 *     joined into one batch on the device first.  The row order of a side is batch order, then row order inside the batch.
 *   - limits: left rows + right rows < 2^32 and output rows < 2^32 (counted in 64 bits: 65 536 x 65 536 equal keys are
 *     refused), else CHQ_ERR_NOT_SUPPORTED with the count; a Utf8 column past int32 offsets:
 *     CHQ_ERR_ARROW_INVALID_ARGUMENT naming it (for the concatenated keys: both key columns).
 *   - output conventions are those of chq_sort_records: ONE batch, `out_device` ARROW_DEVICE_CPU or ARROW_DEVICE_ROCM; on
 *     failure nothing is returned (release == NULL).  The result is bit-identical from run to run.  Every result has the
 *     full schema of its kind, a result of zero rows too.  chq_ctx_last_stats: rows_in = left rows + right rows, rows_out =
 *     the rows returned.
 * The rows and columns per kind; matches(l) = the right rows whose keys all equal those of left row l, ascending (none for a
 * left row with a null key):
 *   CHQ_JOIN_INNER      one row per pair (l, r), r in matches(l), ascending by left row, then by right row.  Every left
 *                       column, then every right column, key columns of both sides included, each with its input field's
 *                       name, type and nullability (duplicate names are allowed: lookups are first-match, aliases
 *                       disambiguate).  An empty side: zero rows.
 *   CHQ_JOIN_LEFT       for each left row ascending: its pairs ascending by right row, or -- it has none -- ONE row whose
 *                       right columns are all null.  Columns as INNER.  No right rows: every left row padded.
 *   CHQ_JOIN_RIGHT      exactly LEFT with the sides exchanged: ascending by right row, then by left row; an unmatched right
 *                       row carries null left columns.  The columns are still left, then right.
 *   CHQ_JOIN_FULL       the rows of LEFT, then every right row that matches no left row, ascending by right row, with every
 *                       left column null.  An empty left side: every right row padded.
 *   CHQ_JOIN_LEFT_SEMI  every left row with at least one match, once, ascending.  Left columns only.
 *   CHQ_JOIN_LEFT_ANTI  every left row with no match, once, ascending -- a left row with a null key among them: this is
 *                       NOT EXISTS, not NOT IN.  Left columns only.  No right rows: every left row.
 *   - padding: the fields of a padded side (the right of LEFT, the left of RIGHT, both of FULL) come out NULLABLE whatever
 *     the input field said; all other fields keep their input nullability.  The slot under a padded null is deterministic:
 *     zero bytes for a fixed width, a 0 bit for Boolean, length 0 for Utf8.  Null counts are exact for every column: the
 *     source's own nulls plus the padding.
 * Out of scope: CROSS joins, non-equality conditions, expressions as keys, coercion between key types.  A call is
 * single-instance; the route to a partitioned or multi-instance join is chq_partition_records on both sides, then one call
 * per partition (for every kind: equal keys share a partition, and a row without a match has none in any other). */
typedef enum chq_join_kind {
  CHQ_JOIN_INNER = 0,
  CHQ_JOIN_LEFT = 1,
  CHQ_JOIN_RIGHT = 2,
  CHQ_JOIN_FULL = 3,
  CHQ_JOIN_LEFT_SEMI = 4,
  CHQ_JOIN_LEFT_ANTI = 5
} chq_join_kind;
typedef struct chq_join_key {
  const chq_expr* left;    /* column of the left schema */
  const chq_expr* right;   /* column of the right schema */
} chq_join_key;
chq_status chq_join_records(chq_ctx* ctx, int n_left, const struct ArrowDeviceArray* const* left,
                            const struct ArrowSchema* left_schema, const chq_table_aliases* left_aliases, int n_right,
                            const struct ArrowDeviceArray* const* right, const struct ArrowSchema* right_schema,
                            const chq_table_aliases* right_aliases, const chq_join_key* keys, int n_keys, int out_device,
                            struct ArrowDeviceArray* out, struct ArrowSchema* out_schema);   /* kind CHQ_JOIN_INNER */
/* `kind`: a chq_join_kind; any other value: CHQ_ERR_ARROW_INVALID_ARGUMENT */
chq_status chq_join_records_kind(chq_ctx* ctx, int n_left, const struct ArrowDeviceArray* const* left,
                                 const struct ArrowSchema* left_schema, const chq_table_aliases* left_aliases, int n_right,
                                 const struct ArrowDeviceArray* const* right, const struct ArrowSchema* right_schema,
                                 const chq_table_aliases* right_aliases, const chq_join_key* keys, int n_keys, int kind,
                                 int out_device, struct ArrowDeviceArray* out, struct ArrowSchema* out_schema);

/* ---- Hash partitioning of a group of record batches by key columns --------------------------------
 * The primitive that lets a keyed operator run on more than one instance: the rows of the group are cut into `n_partitions`
 * batches so that ALL ROWS WITH EQUAL KEYS LAND IN THE SAME OUTPUT.  Rank p then joins partition p of the left input with
 * partition p of the right, and a GROUP BY group lies wholly inside one partition.
 *   - input: a group of n >= 1 batches of one schema, host or device resident, sliced or empty; it is joined into one batch
 *     on the device first, as chq_sort_records does.
 *   - keys: one or more columns (Identifier / CompoundIdentifier) resolved exactly like a sort key (a missing column: the
 *     evaluator's status; any other expression: CHQ_ERR_NOT_SUPPORTED).  The key types are those of ORDER BY and JOIN; a type
 *     without an order (FixedSizeBinary, ...): CHQ_ERR_NOT_SUPPORTED naming the column and its Arrow type.  No key:
 *     CHQ_ERR_ARROW_INVALID_ARGUMENT.
 *   - `n_partitions` in [1, 256], else CHQ_ERR_ARROW_INVALID_ARGUMENT (and `outs` is not touched); 2^32 rows or more:
 *     CHQ_ERR_NOT_SUPPORTED.
 *   - output: exactly `n_partitions` batches with the input schema (names, types, nullability).  Output p holds the rows
 *     whose partition id is p, IN INPUT ORDER (batch order, then row order): the split is stable, every row appears exactly
 *     once, an empty partition is an empty batch with the full schema, and the result is bit-identical from run to run.  All
 *     outputs are slices of ONE gathered batch and share its buffers (null counts as chq_filter_records gives them: exact for
 *     a host result, -1 for a device result's nullable columns).  `out_device` is ARROW_DEVICE_CPU or ARROW_DEVICE_ROCM.  On
 *     failure nothing is returned (release == NULL for every output).
 *   - THE PARTITION ID IS A PINNED FUNCTION OF THE KEY BITS: every rank, and both sides of a join, compute the same one.
 *     All arithmetic is mod 2^64.
 *       fmix64(x):   x ^= x >> 33; x *= 0xFF51AFD7ED558CCD; x ^= x >> 33; x *= 0xC4CEB9FE1A85EC53; x ^= x >> 33
 *       V(null)    = 0
 *       V(value):    acc = fmix64(L + 1), L the value's byte length (the width of a fixed-width type; 1 for a Boolean, whose
 *                    value is one byte holding 0 or 1; the string's length for Utf8); then for every 8-byte chunk of the
 *                    value's bytes (little-endian, the last chunk zero-padded) acc = fmix64(acc ^ chunk).  Decimal128 is two
 *                    chunks, low word first.  Values are taken BY BITS, as join and group equality take them: -0 and +0 may
 *                    part, and so may NaNs with different payloads.
 *       row hash:    h = 0x9E3779B97F4A7C15; for each key in the order given h = fmix64(h * 0x9E3779B97F4A7C15 + V)
 *       partition id = ((h >> 32) * n_partitions) >> 32
 *     The Int32 5 and the Int64 5 hash differently: join keys must have identical formats anyway.  Pins (one-key rows, h):
 *     Int32 0 -> 0092d4ed7de0c088, Int32 1 -> 94e150e41a43b226 (partition 4 of 8, 148 of 256), Utf8 "a" ->
 *     8fdebbde62f89937, null -> 3836f0681055a942; the full table is in DESIGN.md section 3.9 and tests/test_partition_host.py.
 *   - chq_ctx_last_stats: rows_in = rows_out = the rows of the group, launches, algorithmic bytes, kernel_ns.
 * Out of scope: expressions as keys, range partitioning, more than 256 partitions per call. */
chq_status chq_partition_records(chq_ctx* ctx, int n_records, const struct ArrowDeviceArray* const* recs,
                                 const struct ArrowSchema* schema, const chq_table_aliases* table_aliases,
                                 const chq_expr* const* keys, int n_keys, int n_partitions, int out_device,
                                 struct ArrowDeviceArray* outs, struct ArrowSchema* out_schemas);

/* Wrap caller-owned device (or host) buffers as a record batch without copying; the buffers must
 * outlive the returned structs, whose release callbacks free only the descriptors. `format` is an
 * Arrow C format string ("i","f","g","l","b","u", ...). */
typedef struct chq_column_desc {
  const char* name;
  const char* format;
  int nullable;
  int64_t null_count;
  int64_t offset;          /* logical offset in elements (Arrow slice offset) */
  const void* validity;    /* NULL when null_count == 0 */
  const void* values;      /* fixed width: values; bool: bitmap; utf8: int32 offsets */
  const void* data;        /* utf8: bytes */
} chq_column_desc;
chq_status chq_wrap_columns(chq_ctx* ctx, const chq_column_desc* cols, int n_cols, int64_t n_rows, int device_type,
                            struct ArrowDeviceArray* out, struct ArrowSchema* out_schema);

#ifdef __cplusplus
}
#endif
#endif /* CHQ_H */
