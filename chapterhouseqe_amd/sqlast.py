"""Host-side mirror of the `sqlparser::ast` subset that ChapterhouseDB's record_utils consume.

The reference hands `sqlparser 0.52` AST nodes (`Expr`, `SelectItem`) to
`compute_value` / `filter_record` / `project_record`
(reference: src/handlers/operator_handler/operators/record_utils/compute_value.rs:57-61,
filter_record.rs:21-25, record_projection.rs:16-20).  These classes carry the same variants and
field names so tests and callers read like the reference's own (`Expr::BinaryOp { left, op, right }`
-> `BinaryOp(left, op, right)`).  Variants compute_value does not implement are kept as
`Unsupported*` nodes so the error path (`ExpressionTypeNotImplemented`, ...) is reproducible.
"""
from __future__ import annotations

import enum
from dataclasses import dataclass
from typing import Optional, Tuple, Union


class BinaryOperator(enum.Enum):
    """sqlparser::ast::BinaryOperator (subset + the ones that must hit the not-implemented arm)."""
    Plus = "Plus"
    Minus = "Minus"
    Multiply = "Multiply"
    Divide = "Divide"
    Modulo = "Modulo"
    StringConcat = "StringConcat"
    Gt = "Gt"
    Lt = "Lt"
    GtEq = "GtEq"
    LtEq = "LtEq"
    Spaceship = "Spaceship"
    Eq = "Eq"
    NotEq = "NotEq"
    And = "And"
    Or = "Or"
    Xor = "Xor"
    BitwiseOr = "BitwiseOr"
    BitwiseAnd = "BitwiseAnd"
    BitwiseXor = "BitwiseXor"


@dataclass(frozen=True)
class Ident:
    value: str
    quote_style: Optional[str] = None


# ---- sqlparser::ast::Value -------------------------------------------------------------------
@dataclass(frozen=True)
class Number:
    """Value::Number(String, bool) -- text kept verbatim; typing happens in compute_value.rs:219-250."""
    text: str
    long: bool = False


@dataclass(frozen=True)
class SingleQuotedString:
    value: str


@dataclass(frozen=True)
class Boolean:
    value: bool


@dataclass(frozen=True)
class UnsupportedValue:
    """Any other Value variant (Null, DoubleQuotedString, HexStringLiteral, ...)."""
    debug: str


Value = Union[Number, SingleQuotedString, Boolean, UnsupportedValue]


# ---- sqlparser::ast::Expr --------------------------------------------------------------------
class Expr:
    pass


@dataclass(frozen=True)
class Identifier(Expr):
    ident: Ident


@dataclass(frozen=True)
class CompoundIdentifier(Expr):
    idents: Tuple[Ident, ...]


@dataclass(frozen=True)
class ValueExpr(Expr):
    """Expr::Value(v)"""
    value: Value


@dataclass(frozen=True)
class BinaryOp(Expr):
    left: Expr
    op: BinaryOperator
    right: Expr


@dataclass(frozen=True)
class Nested(Expr):
    expr: Expr


@dataclass(frozen=True)
class Like(Expr):
    """Expr::Like { negated, expr, pattern, escape_char }: `expr [NOT] LIKE pattern [ESCAPE 'c']`.  The evaluator takes a
    single-quoted string literal as `pattern` (Nested around it allowed); `escape_char` is None or one character."""
    expr: Expr
    pattern: Expr
    negated: bool = False
    escape_char: Optional[str] = None


@dataclass(frozen=True)
class IsNull(Expr):
    """Expr::IsNull(expr) / Expr::IsNotNull(expr) (`negated`)"""
    expr: Expr
    negated: bool = False


@dataclass(frozen=True)
class Case(Expr):
    """Expr::Case { operand, conditions, results, else_result }: `CASE [operand] WHEN c THEN r ... [ELSE e] END`.  With an
    operand (simple CASE) the conditions are the values it is compared with."""
    operand: Optional[Expr]
    conditions: Tuple[Expr, ...]
    results: Tuple[Expr, ...]
    else_result: Optional[Expr] = None


@dataclass(frozen=True)
class InList(Expr):
    """Expr::InList { expr, list, negated }: `expr [NOT] IN (l1, ..)`"""
    expr: Expr
    list: Tuple[Expr, ...]
    negated: bool = False


@dataclass(frozen=True)
class Between(Expr):
    """Expr::Between { expr, negated, low, high }: `expr [NOT] BETWEEN low AND high`"""
    expr: Expr
    negated: bool
    low: Expr
    high: Expr


class CastType(enum.IntEnum):
    """the target of a Cast (include/chq.h: chq_cast_type)"""
    Boolean = 0
    Int8 = 1
    Int16 = 2
    Int32 = 3
    Int64 = 4
    UInt8 = 5
    UInt16 = 6
    UInt32 = 7
    UInt64 = 8
    Float16 = 9
    Float32 = 10
    Float64 = 11
    Utf8 = 12
    Other = 13


@dataclass(frozen=True)
class Cast(Expr):
    """Expr::Cast { kind, expr, data_type }: `CAST(expr AS T)`, `expr::T` and -- `try_cast` -- `TRY_CAST(expr AS T)`"""
    expr: Expr
    data_type: CastType
    try_cast: bool = False

    @property
    def args(self):
        """None, as for every call whose parentheses hold no plain expression list (`Function.args`): before the grammar
        knew the form, `cast(a as int)` parsed as such a call, and code that asks an expression for its call arguments
        (the GROUP BY and window front-ends) keeps getting that answer."""
        return None


class TypedStringType(enum.IntEnum):
    """the data type of a TypedString (include/chq.h: chq_typed_string_kind)"""
    Date = 0
    Timestamp = 1


@dataclass(frozen=True)
class TypedString(Expr):
    """Expr::TypedString { data_type, value }: `DATE '2024-03-01'`, `TIMESTAMP '2024-03-01 00:00:00'`"""
    data_type: TypedStringType
    value: str


@dataclass(frozen=True)
class Extract(Expr):
    """Expr::Extract { field, expr }: `EXTRACT(field FROM expr)`; `field` as written.  It reaches the library as
    `date_part('field', expr)`."""
    field: str
    expr: Expr

    @property
    def args(self):
        """None, like `Cast.args`: `extract(year from ts)` parsed as a call without a plain argument list before"""
        return None


@dataclass(frozen=True)
class UnsupportedExpr(Expr):
    """UnaryOp, Function, Subquery, ... -- compute_value.rs:338-342 rejects them."""
    debug: str


@dataclass(frozen=True)
class WindowSpec:
    """`OVER ( [PARTITION BY e {, e}] [ORDER BY o {, o}] [frame] )`.  `frame` is a `WindowFrame`, resolved by the parser:
    written, or the SQL default (RANGE_TO_CURRENT with ORDER BY, PARTITION without)."""
    partition_by: Tuple["Expr", ...] = ()
    order_by: Tuple["OrderByExpr", ...] = ()
    frame: int = 0


@dataclass(frozen=True, repr=False)
class Function(UnsupportedExpr):
    """Expr::Function: a call `name(args)` / `name(*)`.  compute_value rejects it like every UnsupportedExpr (its debug text
    is `Function(name)`); the GROUP BY front-end reads the aggregate calls of a SELECT list from it.  `args` is None when
    what stands between the parentheses is not a plain expression list (`count(distinct a)`, `cast(a as int)`).  `over`:
    the window the call is evaluated over (`name(args) OVER (...)`), read by `sqlparse.window_plan`."""
    name: str = ""
    args: Optional[Tuple[Expr, ...]] = ()
    star: bool = False
    over: Optional[WindowSpec] = None

    def __repr__(self) -> str:   # the text an enclosing Unsupported node quotes
        return f"UnsupportedExpr(debug={self.debug!r})"


# ---- sqlparser::ast::SelectItem --------------------------------------------------------------
class SelectItem:
    pass


@dataclass(frozen=True)
class Wildcard(SelectItem):
    pass


@dataclass(frozen=True)
class QualifiedWildcard(SelectItem):
    prefix: str


@dataclass(frozen=True)
class UnnamedExpr(SelectItem):
    expr: Expr


@dataclass(frozen=True)
class ExprWithAlias(SelectItem):
    expr: Expr
    alias: Ident


# ---- sqlparser::ast::OrderByExpr ---------------------------------------------------------------
@dataclass(frozen=True)
class OrderByExpr:
    """`expr [ASC|DESC] [NULLS FIRST|LAST]`; None = not written.  The SQL defaults (resolved by `sort_options`):
    ASC, and NULLS LAST for ASC / NULLS FIRST for DESC (PostgreSQL, DataFusion)."""
    expr: Expr
    asc: Optional[bool] = None
    nulls_first: Optional[bool] = None

    def sort_options(self) -> Tuple[bool, bool]:
        """(descending, nulls_first) as the library's sort takes them"""
        asc = True if self.asc is None else self.asc
        return (not asc, (not asc) if self.nulls_first is None else self.nulls_first)


# ---- GROUP BY: one output column (include/chq.h: chq_agg_item) -----------------------------------
class AggKind(enum.IntEnum):
    KEY = 0
    COUNT_STAR = 1
    COUNT = 2
    SUM = 3
    MIN = 4
    MAX = 5
    AVG = 6
    COUNT_DISTINCT = 7


@dataclass(frozen=True)
class AggItem:
    """`KEY`: `key_index` into the GROUP BY keys; `COUNT_STAR`: nothing else; the others: their argument `column`.
    `AVG` is Float64 (integers: the exact total rounded once, over the count; it never overflows); `COUNT_DISTINCT` counts
    the distinct non-null bit patterns of `column`, which may have any type ORDER BY takes as a key."""
    kind: AggKind
    name: str
    key_index: int = -1
    column: Optional[Expr] = None


# ---- window functions: one output column (include/chq.h: chq_window_item) ------------------------
class WindowKind(enum.IntEnum):
    ROW_NUMBER = 0
    RANK = 1
    DENSE_RANK = 2
    LAG = 3
    LEAD = 4
    COUNT_STAR = 5
    COUNT = 6
    SUM = 7
    MIN = 8
    MAX = 9


class WindowFrame(enum.IntEnum):
    PARTITION = 0           # the whole partition
    ROWS_TO_CURRENT = 1     # ROWS BETWEEN UNBOUNDED PRECEDING AND CURRENT ROW
    RANGE_TO_CURRENT = 2    # RANGE BETWEEN UNBOUNDED PRECEDING AND CURRENT ROW: through the row's last peer


@dataclass(frozen=True)
class WindowItem:
    """ROW_NUMBER / RANK / DENSE_RANK: nothing else; LAG / LEAD: `column` and `offset`; COUNT_STAR: `frame`; COUNT / SUM /
    MIN / MAX: `column` and `frame`."""
    kind: WindowKind
    name: str
    column: Optional[Expr] = None
    frame: WindowFrame = WindowFrame.PARTITION
    offset: int = 0


# ---- small constructors used by tests (the reference builds these structs literally) ----------
def ident(name: str) -> Identifier:
    return Identifier(Ident(name))


def compound(*parts: str) -> CompoundIdentifier:
    return CompoundIdentifier(tuple(Ident(p) for p in parts))


def number(text: str, long: bool = False) -> ValueExpr:
    return ValueExpr(Number(text, long))


def string(value: str) -> ValueExpr:
    return ValueExpr(SingleQuotedString(value))


def boolean(value: bool) -> ValueExpr:
    return ValueExpr(Boolean(value))


def binop(left: Expr, op: BinaryOperator, right: Expr) -> BinaryOp:
    return BinaryOp(left, op, right)
