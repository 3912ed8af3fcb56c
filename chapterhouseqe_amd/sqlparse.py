"""Minimal SQL front-end producing the `sqlast` nodes the record kernels consume.

The reference gets its expressions from the third-party `sqlparser 0.52` crate (GenericDialect,
reference: src/planner/logical_planner.rs:228-300; test use: record_utils/test_compute_value.rs:127-148).
That crate is control-plane and out of scope; this module only restates enough of its *expression*
grammar -- tokens, operator precedence (Or 5 < And 10 < Is 17 < Like 19 < comparison 20 < +,- 30 < *,/,% 40), left
associativity, `Nested` for parentheses, `Number` text kept verbatim -- for tests, the bench and the
sample queries (reference: sample_queries/simple.sql) to be written as SQL text.

    <expr> [not] like <expr> [escape '<one character>']      -> Like   (the evaluator wants a string literal as pattern)
    <expr> is [not] null                                     -> IsNull
    <expr> [not] in ( <expr> {, <expr>} )                    -> InList   (comparison precedence)
    <expr> [not] between <low> and <high>                    -> Between  (comparison precedence; <low> and <high> are parsed
                                                                at that precedence, so the `and` belongs to BETWEEN)
    case [<expr>] when <expr> then <expr> {when ..} [else <expr>] end   -> Case
  `case` opens a CASE where `when` or something that can start an expression follows; `when`, `then`, `else` and `end` are
  never implicit aliases (quoted identifiers still are).
  `like`, `not`, `is` and `escape` are operators only where these forms continue (`like` / `not like` in front of something
  that can start an expression, `is` in front of `null` / `not null`, `escape` behind a pattern and in front of a string);
  anywhere else they stay ordinary words, e.g. aliases.  Prefix `not <expr>` stays an UnsupportedExpr.
    date '<string>' | timestamp '<string>'                   -> TypedString (the keyword counts only in front of a string
                                                                literal; anywhere else `date` and `timestamp` are ordinary words)
    extract ( <field> from <expr> )                          -> Extract (sent to the library as date_part('<field>', <expr>))
    cast ( <expr> as <type> ) | try_cast ( <expr> as <type> ) | <expr> :: <type>   -> Cast
  `cast` / `try_cast` open the form only in front of `(`; `::` binds tighter than any binary operator.  <type> is one of
  boolean | bool | tinyint | smallint | int | integer | bigint (each integer name optionally followed by `unsigned`) | real |
  float | double [precision] | varchar | text | string; a length or precision argument and any other name are errors.

    select [distinct] <items> from <func>('<path>') [[as] alias] {[inner] join <func>('<path>') [[as] alias] on <expr>}
        [where <expr>] [group by <column> {, ...}] [having <expr>]
  `distinct` is the keyword right behind `select` where something that can start an expression, or `*`, follows (`select
  distinct from t` selects a column called `distinct`); `having` is never an implicit alias.  The aggregates of a SELECT
  list and of HAVING are count(*), count(c), sum(c), min(c), max(c) and avg(c); `count(distinct c)` is not spelled here
  (AggKind.COUNT_DISTINCT is reached through AggItem).
    a select item may be a window call: <name>(<args>) over ([partition by <column> {, ...}] [order by ...]
        [rows|range between unbounded preceding and current row|unbounded following])
        [order by <expr> [asc|desc] [nulls first|last] {, ...}] [limit <n>]
"""
from __future__ import annotations

import re
from dataclasses import dataclass
from typing import List, Optional, Tuple

from . import sqlast as A

_TOKEN_RE = re.compile(
    r"""\s*(?:
        (?P<comment>--[^\n]*)
      | (?P<number>(?:\d+\.?\d*|\.\d+)(?:[eE][+-]?\d+)?)(?P<long>L)?
      | (?P<string>'(?:[^']|'')*')
      | (?P<qident>"(?:[^"]|"")*")
      | (?P<word>[A-Za-z_][A-Za-z0-9_$]*)
      | (?P<op><>|!=|<=|>=|\|\||==|::|[-+*/%=<>(),.;&|^])
    )""",
    re.X,
)

_PREC_OR, _PREC_AND, _PREC_NOT, _PREC_EQ = 5, 10, 15, 20
_PREC_IS, _PREC_LIKE = 17, 19
_PREC_PIPE, _PREC_CARET, _PREC_AMP, _PREC_XOR = 21, 22, 23, 24
_PREC_PLUS, _PREC_MUL = 30, 40
_PREC_CAST = 50   # postfix `::`: tighter than every binary operator

# the type names of CAST / TRY_CAST / `::` (case-insensitive); the integer names may be followed by UNSIGNED, DOUBLE by PRECISION
_CAST_TYPES = {"BOOLEAN": A.CastType.Boolean, "BOOL": A.CastType.Boolean, "TINYINT": A.CastType.Int8, "SMALLINT": A.CastType.Int16,
               "INT": A.CastType.Int32, "INTEGER": A.CastType.Int32, "BIGINT": A.CastType.Int64, "REAL": A.CastType.Float32,
               "FLOAT": A.CastType.Float32, "DOUBLE": A.CastType.Float64, "VARCHAR": A.CastType.Utf8, "TEXT": A.CastType.Utf8,
               "STRING": A.CastType.Utf8}
_CAST_UNSIGNED = {A.CastType.Int8: A.CastType.UInt8, A.CastType.Int16: A.CastType.UInt16, A.CastType.Int32: A.CastType.UInt32,
                  A.CastType.Int64: A.CastType.UInt64}

_BINOPS = {
    "=": (A.BinaryOperator.Eq, _PREC_EQ), "==": (A.BinaryOperator.Eq, _PREC_EQ),
    "<>": (A.BinaryOperator.NotEq, _PREC_EQ), "!=": (A.BinaryOperator.NotEq, _PREC_EQ),
    "<": (A.BinaryOperator.Lt, _PREC_EQ), "<=": (A.BinaryOperator.LtEq, _PREC_EQ),
    ">": (A.BinaryOperator.Gt, _PREC_EQ), ">=": (A.BinaryOperator.GtEq, _PREC_EQ),
    "+": (A.BinaryOperator.Plus, _PREC_PLUS), "-": (A.BinaryOperator.Minus, _PREC_PLUS),
    "*": (A.BinaryOperator.Multiply, _PREC_MUL), "/": (A.BinaryOperator.Divide, _PREC_MUL),
    "%": (A.BinaryOperator.Modulo, _PREC_MUL), "||": (A.BinaryOperator.StringConcat, _PREC_MUL),
    "|": (A.BinaryOperator.BitwiseOr, _PREC_PIPE), "^": (A.BinaryOperator.BitwiseXor, _PREC_CARET),
    "&": (A.BinaryOperator.BitwiseAnd, _PREC_AMP),
}
_WORD_BINOPS = {"OR": (A.BinaryOperator.Or, _PREC_OR), "AND": (A.BinaryOperator.And, _PREC_AND),
                "XOR": (A.BinaryOperator.Xor, _PREC_XOR)}
_STOP_WORDS = {"FROM", "WHERE", "AS", "GROUP", "HAVING", "ORDER", "LIMIT", "JOIN", "INNER", "ON"}
_CASE_WORDS = {"WHEN", "THEN", "ELSE", "END"}
_OTHER_JOINS = {"LEFT", "RIGHT", "FULL", "OUTER", "CROSS"}


class SqlParseError(ValueError):
    pass


@dataclass(frozen=True)
class TableFunc:
    """`read_files('glob') alias` -- reference: planner OperatorTask::TableFunc { alias, func_name, args }."""
    func_name: str
    args: Tuple[str, ...]
    alias: Optional[str]


@dataclass(frozen=True)
class Join:
    """`[inner] join read_files('glob') alias on <cond>`"""
    table: TableFunc
    on: A.Expr


@dataclass(frozen=True)
class Select:
    projection: Tuple[A.SelectItem, ...]
    from_: Optional[TableFunc]
    selection: Optional[A.Expr]
    order_by: Tuple[A.OrderByExpr, ...] = ()
    limit: Optional[int] = None
    group_by: Tuple[A.Expr, ...] = ()
    joins: Tuple[Join, ...] = ()
    having: Optional[A.Expr] = None
    distinct: bool = False


def _tokenize(text: str) -> List[Tuple[str, str]]:
    out, pos = [], 0
    while pos < len(text):
        m = _TOKEN_RE.match(text, pos)
        if not m or m.end() == pos:
            if text[pos:].strip() == "":
                break
            raise SqlParseError(f"cannot tokenize at: {text[pos:pos + 20]!r}")
        pos = m.end()
        if m.group("comment") is not None:
            continue
        if m.group("number") is not None:
            out.append(("numberL" if m.group("long") else "number", m.group("number")))
        elif m.group("string") is not None:
            out.append(("string", m.group("string")[1:-1].replace("''", "'")))
        elif m.group("qident") is not None:
            out.append(("qident", m.group("qident")[1:-1].replace('""', '"')))
        elif m.group("word") is not None:
            out.append(("word", m.group("word")))
        else:
            out.append(("op", m.group("op")))
    return out


class _Parser:
    def __init__(self, toks):
        self.toks, self.i = toks, 0

    def peek(self):
        return self.toks[self.i] if self.i < len(self.toks) else ("eof", "")

    def next(self):
        t = self.peek()
        self.i += 1
        return t

    def accept_op(self, op):
        if self.peek() == ("op", op):
            self.i += 1
            return True
        return False

    def accept_word(self, w):
        k, v = self.peek()
        if k == "word" and v.upper() == w:
            self.i += 1
            return True
        return False

    def expect_op(self, op):
        if not self.accept_op(op):
            raise SqlParseError(f"expected {op!r}, found {self.peek()[1]!r}")

    # ---- expressions: sqlparser Parser::parse_subexpr ------------------------------------------
    def _word_at(self, j):
        k, v = self.toks[self.i + j] if self.i + j < len(self.toks) else ("eof", "")
        return v.upper() if k == "word" else None

    def _starts_expr(self, j) -> bool:
        k, v = self.toks[self.i + j] if self.i + j < len(self.toks) else ("eof", "")
        if k == "word":
            return v.upper() not in _STOP_WORDS and v.upper() not in _CASE_WORDS
        return k in ("number", "numberL", "string", "qident") or (k == "op" and v in ("(", "-", "+"))

    def _infix_words(self):
        """the word operator at the cursor: (node kind, negated, tokens it takes, precedence), or None"""
        w = self._word_at(0)
        if w == "LIKE" and self._starts_expr(1):
            return ("like", False, 1, _PREC_LIKE)
        if w == "NOT" and self._word_at(1) == "LIKE" and self._starts_expr(2):
            return ("like", True, 2, _PREC_LIKE)
        if w == "IS" and self._word_at(1) == "NULL":
            return ("is", False, 2, _PREC_IS)
        if w == "IS" and self._word_at(1) == "NOT" and self._word_at(2) == "NULL":
            return ("is", True, 3, _PREC_IS)
        neg = 1 if w == "NOT" else 0
        if self._word_at(neg) == "IN" and self.i + neg + 1 < len(self.toks) and self.toks[self.i + neg + 1] == ("op", "("):
            return ("in", bool(neg), neg + 1, _PREC_EQ)
        if self._word_at(neg) == "BETWEEN" and self._starts_expr(neg + 1):
            return ("between", bool(neg), neg + 1, _PREC_EQ)
        return None

    def next_precedence(self):
        k, v = self.peek()
        infix = self._infix_words()
        if infix:
            return infix[3]
        if k == "op" and v == "::":
            return _PREC_CAST
        if k == "op" and v in _BINOPS:
            return _BINOPS[v][1]
        if k == "word" and v.upper() in _WORD_BINOPS:
            return _WORD_BINOPS[v.upper()][1]
        return 0

    def parse_expr(self, precedence=0) -> A.Expr:
        expr = self.parse_prefix()
        while True:
            nxt = self.next_precedence()
            if precedence >= nxt:
                break
            infix = self._infix_words()
            if infix:   # sqlparser Parser::parse_infix: Keyword::LIKE / NOT / IS
                kind, negated, ntok, _ = infix
                self.i += ntok
                if kind == "is":
                    expr = A.IsNull(expr, negated)
                    continue
                if kind == "in":   # Keyword::IN: a parenthesised expression list (a subquery is not part of this grammar)
                    self.expect_op("(")
                    items = [self.parse_expr(0)]
                    while self.accept_op(","):
                        items.append(self.parse_expr(0))
                    self.expect_op(")")
                    expr = A.InList(expr, tuple(items), negated)
                    continue
                if kind == "between":   # Keyword::BETWEEN: parse_between
                    low = self.parse_expr(_PREC_EQ)
                    if not self.accept_word("AND"):
                        raise SqlParseError(f"expected AND after the low bound of BETWEEN, found {self.peek()[1]!r}")
                    high = self.parse_expr(_PREC_EQ)
                    expr = A.Between(expr, negated, low, high)
                    continue
                pattern = self.parse_expr(_PREC_LIKE)
                escape = None
                if self._word_at(0) == "ESCAPE" and self.i + 1 < len(self.toks) and self.toks[self.i + 1][0] == "string":
                    escape = self.toks[self.i + 1][1]
                    self.i += 2
                    if len(escape) != 1:
                        raise SqlParseError(f"ESCAPE takes one character, found {escape!r}")
                expr = A.Like(expr, pattern, negated, escape)
                continue
            k, v = self.next()
            if (k, v) == ("op", "::"):   # Expr::Cast { kind: DoubleColon }: the same as CAST
                expr = A.Cast(expr, self._data_type(), False)
                continue
            op = _BINOPS[v][0] if k == "op" else _WORD_BINOPS[v.upper()][0]
            right = self.parse_expr(nxt)
            expr = A.BinaryOp(expr, op, right)
        return expr

    def parse_prefix(self) -> A.Expr:
        k, v = self.next()
        if k == "number":
            return A.ValueExpr(A.Number(v, False))
        if k == "numberL":
            return A.ValueExpr(A.Number(v, True))
        if k == "string":
            return A.ValueExpr(A.SingleQuotedString(v))
        if k == "op" and v == "(":
            inner = self.parse_expr(0)
            self.expect_op(")")
            return A.Nested(inner)
        if k == "op" and v in ("-", "+"):
            inner = self.parse_expr(_PREC_MUL)
            return A.UnsupportedExpr(f"UnaryOp {{ op: {'Minus' if v == '-' else 'Plus'}, expr: {inner!r} }}")
        if k == "word":
            up = v.upper()
            if up == "TRUE":
                return A.ValueExpr(A.Boolean(True))
            if up == "FALSE":
                return A.ValueExpr(A.Boolean(False))
            if up == "NULL":
                return A.ValueExpr(A.UnsupportedValue("Null"))
            if up == "NOT":
                inner = self.parse_expr(_PREC_NOT)
                return A.UnsupportedExpr(f"UnaryOp {{ op: Not, expr: {inner!r} }}")
            # (`case + 1` and `case - 1` stay arithmetic on a column of that name)
            if up == "CASE" and (self._word_at(0) == "WHEN" or (self._starts_expr(0) and self.peek() not in (("op", "-"), ("op", "+")))):
                return self._case()
            if up in ("CAST", "TRY_CAST") and self.peek() == ("op", "("):
                return self._cast(up == "TRY_CAST")
            # Expr::TypedString: the keyword counts only in front of a string literal; elsewhere `date` / `timestamp` are words
            if up in ("DATE", "TIMESTAMP") and self.peek()[0] == "string":
                return A.TypedString(A.TypedStringType.Date if up == "DATE" else A.TypedStringType.Timestamp, self.next()[1])
            if up == "EXTRACT" and self.peek() == ("op", "("):
                ex = self._extract()
                if ex is not None:
                    return ex
            if self.peek() == ("op", "("):
                return self._function_call(v)
            return self._identifier_tail(A.Ident(v))
        if k == "qident":
            return self._identifier_tail(A.Ident(v, '"'))
        raise SqlParseError(f"unexpected token {v!r}")

    def _cast(self, try_cast: bool) -> A.Expr:
        """`( expr AS type )` behind CAST / TRY_CAST: sqlparser Parser::parse_cast_expr / parse_try_cast_expr"""
        self.expect_op("(")
        inner = self.parse_expr(0)
        if not self.accept_word("AS"):
            raise SqlParseError(f"expected AS in {'TRY_CAST' if try_cast else 'CAST'}, found {self.peek()[1]!r}")
        to = self._data_type()
        self.expect_op(")")
        return A.Cast(inner, to, try_cast)

    def _extract(self) -> Optional[A.Expr]:
        """`( field FROM expr )` behind EXTRACT: sqlparser Parser::parse_extract_expr.  `field` is a word or a string literal.
        Anything else between the parentheses: None, and the text parses as a call like before."""
        start = self.i
        self.expect_op("(")
        k, field = self.next()
        if k in ("word", "string") and self.accept_word("FROM"):
            inner = self.parse_expr(0)
            self.expect_op(")")
            return A.Extract(field, inner)
        self.i = start
        return None

    def _data_type(self) -> A.CastType:
        k, v = self.next()
        if k != "word" or v.upper() not in _CAST_TYPES:
            raise SqlParseError(f"{v!r} is not a type CAST knows: {', '.join(sorted(_CAST_TYPES))}")
        to = _CAST_TYPES[v.upper()]
        if to in _CAST_UNSIGNED and self.accept_word("UNSIGNED"):
            to = _CAST_UNSIGNED[to]
        if v.upper() == "DOUBLE":
            self.accept_word("PRECISION")
        if self.peek() == ("op", "("):
            raise SqlParseError(f"a length or precision argument of {v} is not supported")
        return to

    def _case(self) -> A.Expr:
        """sqlparser Parser::parse_case_expr, behind the CASE keyword"""
        operand = None if self._word_at(0) == "WHEN" else self.parse_expr(0)
        conditions, results = [], []
        while self.accept_word("WHEN"):
            conditions.append(self.parse_expr(0))
            if not self.accept_word("THEN"):
                raise SqlParseError(f"expected THEN after the condition of WHEN, found {self.peek()[1]!r}")
            results.append(self.parse_expr(0))
        if not conditions:
            raise SqlParseError(f"expected WHEN after CASE, found {self.peek()[1]!r}")
        else_result = self.parse_expr(0) if self.accept_word("ELSE") else None
        if not self.accept_word("END"):
            raise SqlParseError(f"expected END to close CASE, found {self.peek()[1]!r}")
        return A.Case(operand, tuple(conditions), tuple(results), else_result)

    def _function_call(self, name: str) -> A.Expr:
        """`name ( [* | expr {, expr}] )`; anything else between the parentheses is skipped (args None).  compute_value
        rejects every call, so the reference's evaluator sees `Function(name)` whatever the arguments are.  `substring(s from p
        [for n])` is the comma form spelled differently: the same `Function` with args (s, p[, n]).  The position and length
        of substring / substr may carry a sign (`-3`): they are integer literals, kept as one Number."""
        start = self.i
        args, star = None, False
        try:
            self.expect_op("(")
            if self.accept_op("*"):
                star, parsed = True, []
            elif self.peek() == ("op", ")"):
                parsed = []
            elif name.lower() in ("substring", "substr"):
                parsed = [self.parse_expr(0)]
                if name.lower() == "substring" and self.accept_word("FROM"):
                    parsed.append(self._signed_number_or_expr())
                    if self.accept_word("FOR"):
                        parsed.append(self._signed_number_or_expr())
                else:
                    while self.accept_op(","):
                        parsed.append(self._signed_number_or_expr())
            else:
                parsed = [self.parse_expr(0)]
                while self.accept_op(","):
                    parsed.append(self.parse_expr(0))
            self.expect_op(")")
            args = tuple(parsed)
        except SqlParseError:
            self.i, star, depth = start, False, 0
            while True:
                kk, vv = self.next()
                if kk == "eof":
                    raise SqlParseError("unterminated function call")
                if (kk, vv) == ("op", "("):
                    depth += 1
                if (kk, vv) == ("op", ")"):
                    depth -= 1
                    if depth == 0:
                        break
        over = self._window_spec() if self.accept_word("OVER") else None
        return A.Function(f"Function({name})", name, args, star, over)

    def _signed_number_or_expr(self) -> A.Expr:
        """an argument that is `[-|+] number` alone becomes that signed Number; anything else parses as any expression"""
        k, v = self.peek()
        if k == "op" and v in ("-", "+") and self.i + 2 < len(self.toks) and self.toks[self.i + 1][0] == "number" and \
                (self.toks[self.i + 2] in (("op", ","), ("op", ")")) or
                 (self.toks[self.i + 2][0] == "word" and self.toks[self.i + 2][1].upper() == "FOR")):
            self.i += 2
            return A.ValueExpr(A.Number(("-" if v == "-" else "") + self.toks[self.i - 1][1], False))
        return self.parse_expr(0)

    def _window_spec(self) -> A.WindowSpec:
        """`( [PARTITION BY e {, e}] [ORDER BY o {, o}] [ROWS | RANGE BETWEEN UNBOUNDED PRECEDING AND CURRENT ROW |
        UNBOUNDED FOLLOWING] )`; the default frame is SQL's: RANGE ... CURRENT ROW with ORDER BY, the partition without."""
        self.expect_op("(")
        partition_by: List[A.Expr] = []
        order_by: List[A.OrderByExpr] = []
        if self.accept_word("PARTITION"):
            if not self.accept_word("BY"):
                raise SqlParseError(f"expected BY after PARTITION, found {self.peek()[1]!r}")
            partition_by.append(self.parse_expr(0))
            while self.accept_op(","):
                partition_by.append(self.parse_expr(0))
        if self.accept_word("ORDER"):
            if not self.accept_word("BY"):
                raise SqlParseError(f"expected BY after ORDER, found {self.peek()[1]!r}")
            order_by.append(self.parse_order_by_expr())
            while self.accept_op(","):
                order_by.append(self.parse_order_by_expr())
        frame = A.WindowFrame.RANGE_TO_CURRENT if order_by else A.WindowFrame.PARTITION
        k, v = self.peek()
        if k == "word" and v.upper() in ("ROWS", "RANGE", "GROUPS"):
            unit = self.next()[1].upper()
            words = []
            while self.peek()[0] not in ("eof",) and self.peek() != ("op", ")"):
                words.append(self.next()[1].upper())
            text = " ".join(words)
            if unit != "GROUPS" and text == "BETWEEN UNBOUNDED PRECEDING AND CURRENT ROW":
                frame = A.WindowFrame.ROWS_TO_CURRENT if unit == "ROWS" else A.WindowFrame.RANGE_TO_CURRENT
            elif unit != "GROUPS" and text == "BETWEEN UNBOUNDED PRECEDING AND UNBOUNDED FOLLOWING":
                frame = A.WindowFrame.PARTITION
            else:
                raise SqlParseError(f"window frame {unit} {text} is not supported: only BETWEEN UNBOUNDED PRECEDING AND "
                                    "CURRENT ROW | UNBOUNDED FOLLOWING")
        if not self.accept_op(")"):
            raise SqlParseError(f"expected ')' to close OVER (...), found {self.peek()[1]!r}")
        return A.WindowSpec(tuple(partition_by), tuple(order_by), frame)

    def _identifier_tail(self, first: A.Ident) -> A.Expr:
        parts = [first]
        while self.peek() == ("op", "."):
            self.next()
            k, v = self.next()
            if k == "word":
                parts.append(A.Ident(v))
            elif k == "qident":
                parts.append(A.Ident(v, '"'))
            else:
                raise SqlParseError("expected identifier after '.'")
        if len(parts) == 1:
            return A.Identifier(parts[0])
        return A.CompoundIdentifier(tuple(parts))

    # ---- select ---------------------------------------------------------------------------------
    def parse_select_item(self) -> A.SelectItem:
        if self.accept_op("*"):
            return A.Wildcard()
        # qualified wildcard: ident . *
        if self.peek()[0] in ("word", "qident") and self.i + 2 < len(self.toks) + 1:
            j = self.i
            if (j + 2 < len(self.toks) and self.toks[j + 1] == ("op", ".") and self.toks[j + 2] == ("op", "*")):
                prefix = self.toks[j][1]
                self.i += 3
                return A.QualifiedWildcard(prefix)
        expr = self.parse_expr(0)
        if self.accept_word("AS"):
            k, v = self.next()
            if k not in ("word", "qident"):
                raise SqlParseError("expected alias after AS")
            return A.ExprWithAlias(expr, A.Ident(v, '"' if k == "qident" else None))
        k, v = self.peek()
        if k == "word" and v.upper() not in _STOP_WORDS and v.upper() not in _CASE_WORDS:
            self.next()
            return A.ExprWithAlias(expr, A.Ident(v))
        return A.UnnamedExpr(expr)

    def reject_other_joins(self) -> None:
        """LEFT / RIGHT / FULL / OUTER / CROSS in front of JOIN (as an alias elsewhere they are ordinary words)"""
        j = self.i
        while j < len(self.toks) and self.toks[j][0] == "word" and self.toks[j][1].upper() in _OTHER_JOINS:
            j += 1
        if j > self.i and j < len(self.toks) and self.toks[j][0] == "word" and self.toks[j][1].upper() == "JOIN":
            kind = " ".join(t[1].upper() for t in self.toks[self.i:j])
            raise SqlParseError(f"{kind} JOIN is not supported: only INNER JOIN is supported")

    def parse_table_func(self, after: str) -> TableFunc:
        k, name = self.next()
        if k != "word":
            raise SqlParseError(f"expected table function or table name after {after}")
        args: List[str] = []
        if self.accept_op("("):
            while not self.accept_op(")"):
                kk, vv = self.next()
                if kk == "eof":
                    raise SqlParseError("unterminated table function")
                if kk == "string":
                    args.append(vv)
        self.reject_other_joins()
        alias = None
        if self.accept_word("AS"):
            alias = self.next()[1]
        else:
            k2, v2 = self.peek()
            if k2 == "word" and v2.upper() not in _STOP_WORDS:
                alias = self.next()[1]
        return TableFunc(name, tuple(args), alias)

    def parse_select(self) -> Select:
        if not self.accept_word("SELECT"):
            raise SqlParseError("expected SELECT")
        distinct = False
        if self._word_at(0) == "DISTINCT" and (self._starts_expr(1) or (self.i + 1 < len(self.toks) and self.toks[self.i + 1] == ("op", "*"))):
            self.i += 1
            distinct = True
        items = [self.parse_select_item()]
        while self.accept_op(","):
            items.append(self.parse_select_item())
        from_ = None
        joins: List[Join] = []
        if self.accept_word("FROM"):
            from_ = self.parse_table_func("FROM")
            while True:
                self.reject_other_joins()
                inner = self.accept_word("INNER")
                if not self.accept_word("JOIN"):
                    if inner:
                        raise SqlParseError(f"expected JOIN after INNER, found {self.peek()[1]!r}")
                    break
                table = self.parse_table_func("JOIN")
                if not self.accept_word("ON"):
                    raise SqlParseError(f"expected ON after the joined table, found {self.peek()[1]!r}")
                joins.append(Join(table, self.parse_expr(0)))
        selection = None
        if self.accept_word("WHERE"):
            selection = self.parse_expr(0)
        group_by: List[A.Expr] = []
        if self.accept_word("GROUP"):
            if not self.accept_word("BY"):
                raise SqlParseError(f"expected BY after GROUP, found {self.peek()[1]!r}")
            group_by.append(self.parse_expr(0))
            while self.accept_op(","):
                group_by.append(self.parse_expr(0))
        having = self.parse_expr(0) if self.accept_word("HAVING") else None
        order_by: List[A.OrderByExpr] = []
        if self.accept_word("ORDER"):
            if not self.accept_word("BY"):
                raise SqlParseError(f"expected BY after ORDER, found {self.peek()[1]!r}")
            order_by.append(self.parse_order_by_expr())
            while self.accept_op(","):
                order_by.append(self.parse_order_by_expr())
        limit = None
        if self.accept_word("LIMIT"):
            k, v = self.next()
            if k != "number" or not v.isdigit():
                raise SqlParseError(f"expected a non-negative integer after LIMIT, found {v!r}")
            limit = int(v)
        self.accept_op(";")
        return Select(tuple(items), from_, selection, tuple(order_by), limit, tuple(group_by), tuple(joins), having, distinct)

    def parse_order_by_expr(self) -> A.OrderByExpr:
        """sqlparser Parser::parse_order_by_expr"""
        expr = self.parse_expr(0)
        asc = True if self.accept_word("ASC") else (False if self.accept_word("DESC") else None)
        nulls_first = None
        if self.accept_word("NULLS"):
            if self.accept_word("FIRST"):
                nulls_first = True
            elif self.accept_word("LAST"):
                nulls_first = False
            else:
                raise SqlParseError(f"expected FIRST or LAST after NULLS, found {self.peek()[1]!r}")
        return A.OrderByExpr(expr, asc, nulls_first)


# ---- GROUP BY: the SELECT list as keys and output items -----------------------------------------------
_AGGREGATES = {"count": A.AggKind.COUNT, "sum": A.AggKind.SUM, "min": A.AggKind.MIN, "max": A.AggKind.MAX, "avg": A.AggKind.AVG}


def _expr_text(e: A.Expr) -> str:
    if isinstance(e, A.Identifier):
        return e.ident.value
    if isinstance(e, A.CompoundIdentifier):
        return ".".join(i.value for i in e.idents)
    if isinstance(e, A.Function):
        call = f"{e.name}({'*' if e.star else ', '.join(_expr_text(a) for a in (e.args or ()))})"
        return call if e.over is None else f"{call} over ({_window_text(e.over)})"
    if isinstance(e, A.ValueExpr) and isinstance(e.value, A.Number):
        return e.value.text
    return repr(e)


def is_aggregate_call(e: A.Expr) -> bool:
    return isinstance(e, A.Function) and e.name.lower() in _AGGREGATES and e.over is None


def aggregate_plan(select: Select):
    """A `Select` with GROUP BY or aggregate calls -> `(keys, items)` as `record_utils.aggregate_record(s)` takes them
    (None: the statement has neither).  Every SELECT item must be a GROUP BY key or one of count(*), count(c), sum(c),
    min(c), max(c), avg(c) (names case-insensitive); an item is named by its alias, else a key by its column name and an
    aggregate by its lower-cased call text.  A HAVING clause is ignored here: `having_plan` builds on this result.
    `select distinct a, b` is GROUP BY a, b with one KEY item each -- the rows come out in key order, which is a property
    of this operator, not something SQL promises -- and takes plain columns only."""
    exprs = [(f.expr if isinstance(f, (A.UnnamedExpr, A.ExprWithAlias)) else None) for f in select.projection]
    if select.distinct:
        return _distinct_plan(select, exprs)
    if not select.group_by and not any(e is not None and is_aggregate_call(e) for e in exprs):
        return None
    keys = tuple(select.group_by)
    items = []
    for f, e in zip(select.projection, exprs):
        if e is None:
            raise SqlParseError("a wildcard cannot be selected together with GROUP BY or an aggregate")
        alias = f.alias.value if isinstance(f, A.ExprWithAlias) else None
        if is_aggregate_call(e):
            kind = _AGGREGATES[e.name.lower()]
            name = alias if alias is not None else _expr_text(e).lower()
            if e.star:
                if kind != A.AggKind.COUNT:
                    raise SqlParseError(f"{e.name}(*) is not an aggregate; only count(*) takes '*'")
                items.append(A.AggItem(A.AggKind.COUNT_STAR, name))
            elif e.args is None or len(e.args) != 1:
                raise SqlParseError(f"{e.name} takes exactly one column: {_expr_text(e) if e.args is not None else e.name + '(...)'}")
            else:
                items.append(A.AggItem(kind, name, -1, e.args[0]))
        elif e in keys:
            name = alias if alias is not None else (e.ident.value if isinstance(e, A.Identifier) else
                                                    e.idents[-1].value if isinstance(e, A.CompoundIdentifier) else _expr_text(e))
            items.append(A.AggItem(A.AggKind.KEY, name, keys.index(e)))
        else:
            raise SqlParseError(f"SELECT item {_expr_text(e)} is neither a GROUP BY key nor an aggregate")
    return keys, tuple(items)


def _column_tail(e: A.Expr) -> str:
    return e.ident.value if isinstance(e, A.Identifier) else e.idents[-1].value


def _distinct_plan(select: Select, exprs):
    if select.group_by or select.having is not None:
        raise SqlParseError("SELECT DISTINCT cannot be combined with GROUP BY or HAVING")
    items = []
    for f, e in zip(select.projection, exprs):
        if e is None:
            raise SqlParseError("SELECT DISTINCT takes plain columns, not a wildcard")
        if is_aggregate_call(e) or _has_window_call(e):
            raise SqlParseError(f"SELECT DISTINCT cannot be combined with aggregates or window calls: {_expr_text(e)}")
        if not isinstance(e, (A.Identifier, A.CompoundIdentifier)):
            raise SqlParseError(f"SELECT DISTINCT takes plain columns, not {_term_text(e)}")
        items.append(A.AggItem(A.AggKind.KEY, f.alias.value if isinstance(f, A.ExprWithAlias) else _column_tail(e), len(items)))
    return tuple(exprs), tuple(items)


def having_plan(select: Select):
    """A `Select` with HAVING -> `(keys, items, predicate, n_visible)` (None: the statement has no HAVING).  `keys` and
    `items[:n_visible]` are `aggregate_plan`'s.  `predicate` is the HAVING expression with every aggregate call (count(*),
    count / sum / min / max / avg of one column) and every GROUP BY key column replaced by an identifier of an output column
    of the aggregate: a visible item of the same kind and argument when its output name is unique among the items, else a
    hidden item `__having_<k>` appended behind the visible ones.  The statement runs as aggregate(all items), then
    `filter_record(predicate)` over that result (null drops the row), then, with hidden items, a projection to the first
    `n_visible` columns.  The statement must be an aggregate statement by its SELECT list and GROUP BY (`aggregate_plan` is
    not None): aggregates that stand in HAVING alone do not make it one -- without GROUP BY there is no key, so no SELECT
    item other than an aggregate could be selected next to them."""
    if select.having is None:
        return None
    plan = aggregate_plan(select)
    if plan is None:
        exprs = [(f.expr if isinstance(f, (A.UnnamedExpr, A.ExprWithAlias)) else None) for f in select.projection]
        if any(e is not None and _has_window_call(e) for e in exprs):
            raise SqlParseError("HAVING cannot be combined with window calls")
        raise SqlParseError("HAVING needs GROUP BY or an aggregate in the SELECT list (an aggregate in HAVING alone does not "
                            "group the statement: its SELECT items are neither keys nor aggregates)")
    keys, visible = plan
    items = list(visible)

    def column_for(kind, key_index=-1, column=None) -> A.Expr:
        for it in items:
            if (it.kind, it.key_index, it.column) == (kind, key_index, column) and sum(o.name == it.name for o in items) == 1:
                return A.Identifier(A.Ident(it.name))
        k = len(items) - len(visible)
        while any(o.name == f"__having_{k}" for o in items):
            k += 1
        items.append(A.AggItem(kind, f"__having_{k}", key_index, column))
        return A.Identifier(A.Ident(items[-1].name))

    def rewrite(e: A.Expr) -> A.Expr:
        if isinstance(e, A.Function):
            if e.over is not None:
                raise SqlParseError(f"a window call cannot stand in HAVING: {_expr_text(e)}")
            if not is_aggregate_call(e):   # a scalar function: the evaluator's business, over rewritten arguments
                return e if e.args is None else A.Function(e.debug, e.name, tuple(rewrite(x) for x in e.args), e.star, None)
            kind = _AGGREGATES[e.name.lower()]
            if e.star:
                if kind != A.AggKind.COUNT:
                    raise SqlParseError(f"{e.name}(*) is not an aggregate; only count(*) takes '*'")
                return column_for(A.AggKind.COUNT_STAR)
            if e.args is None or len(e.args) != 1 or not isinstance(e.args[0], (A.Identifier, A.CompoundIdentifier)):
                raise SqlParseError(f"{e.name} in HAVING takes exactly one plain column: "
                                    f"{_expr_text(e) if e.args is not None else e.name + '(...)'}")
            return column_for(kind, -1, e.args[0])
        if isinstance(e, (A.Identifier, A.CompoundIdentifier)):
            if e not in keys:
                raise SqlParseError(f"column {_expr_text(e)} in HAVING is neither a GROUP BY key nor inside an aggregate")
            return column_for(A.AggKind.KEY, keys.index(e))
        if isinstance(e, A.BinaryOp):
            return A.BinaryOp(rewrite(e.left), e.op, rewrite(e.right))
        if isinstance(e, A.Nested):
            return A.Nested(rewrite(e.expr))
        if isinstance(e, A.IsNull):
            return A.IsNull(rewrite(e.expr), e.negated)
        if isinstance(e, A.Like):
            return A.Like(rewrite(e.expr), rewrite(e.pattern), e.negated, e.escape_char)
        if isinstance(e, A.InList):
            return A.InList(rewrite(e.expr), tuple(rewrite(x) for x in e.list), e.negated)
        if isinstance(e, A.Between):
            return A.Between(rewrite(e.expr), e.negated, rewrite(e.low), rewrite(e.high))
        if isinstance(e, A.Cast):
            return A.Cast(rewrite(e.expr), e.data_type, e.try_cast)
        if isinstance(e, A.Extract):
            return A.Extract(e.field, rewrite(e.expr))
        if isinstance(e, A.Case):
            return A.Case(None if e.operand is None else rewrite(e.operand), tuple(rewrite(x) for x in e.conditions),
                          tuple(rewrite(x) for x in e.results), None if e.else_result is None else rewrite(e.else_result))
        return e   # literals, and what the evaluator rejects by itself

    predicate = rewrite(select.having)
    return keys, tuple(items), predicate, len(visible)


# ---- window functions: the SELECT list as one window call's items ------------------------------------------------------
_WINDOW_KINDS = {"row_number": A.WindowKind.ROW_NUMBER, "rank": A.WindowKind.RANK, "dense_rank": A.WindowKind.DENSE_RANK,
                 "lag": A.WindowKind.LAG, "lead": A.WindowKind.LEAD, "count": A.WindowKind.COUNT, "sum": A.WindowKind.SUM,
                 "min": A.WindowKind.MIN, "max": A.WindowKind.MAX}
_FRAME_TEXT = {A.WindowFrame.PARTITION: "range between unbounded preceding and unbounded following",
               A.WindowFrame.ROWS_TO_CURRENT: "rows between unbounded preceding and current row",
               A.WindowFrame.RANGE_TO_CURRENT: "range between unbounded preceding and current row"}


def _window_text(w: A.WindowSpec) -> str:
    parts = []
    if w.partition_by:
        parts.append("partition by " + ", ".join(_expr_text(e) for e in w.partition_by))
    if w.order_by:
        def key(o: A.OrderByExpr) -> str:
            return _expr_text(o.expr) + ("" if o.asc is None else " asc" if o.asc else " desc") + \
                ("" if o.nulls_first is None else " nulls first" if o.nulls_first else " nulls last")
        parts.append("order by " + ", ".join(key(o) for o in w.order_by))
    parts.append(_FRAME_TEXT[A.WindowFrame(w.frame)])
    return " ".join(parts)


def _has_window_call(e) -> bool:
    if isinstance(e, A.Function):
        return e.over is not None or any(_has_window_call(a) for a in (e.args or ()))
    if isinstance(e, A.BinaryOp):
        return _has_window_call(e.left) or _has_window_call(e.right)
    if isinstance(e, A.Nested):
        return _has_window_call(e.expr)
    return False


def window_plan(select: Select):
    """A `Select` whose SELECT list holds window calls (`fn(...) over (...)`) -> `(partition_by, order_by, items, projection)`:
    the first three as `record_utils.window_record(s)` takes them, `projection` the SELECT list with every window call
    replaced by an identifier of its output column (its alias, else its lower-cased call text without the OVER clause) for `project_record` to
    finish the statement on the window call's result.  None: no call has OVER.  Every window call must be a whole SELECT
    item, all of them must share PARTITION BY and ORDER BY (their frames may differ), and they cannot be mixed with
    GROUP BY or plain aggregates.  row_number() / rank() / dense_rank() take no argument, lag / lead a column and an
    optional integer literal (default 1), count(*) / count / sum / min / max one column."""
    exprs = [(f.expr if isinstance(f, (A.UnnamedExpr, A.ExprWithAlias)) else None) for f in select.projection]
    if not any(e is not None and _has_window_call(e) for e in exprs):
        return None
    if select.group_by or any(e is not None and is_aggregate_call(e) for e in exprs):
        raise SqlParseError("window calls cannot be selected together with GROUP BY or plain aggregates")
    spec = None
    items, projection = [], []
    for f, e in zip(select.projection, exprs):
        if e is None or not _has_window_call(e):
            projection.append(f)
            continue
        if not (isinstance(e, A.Function) and e.over is not None) or any(_has_window_call(a) for a in (e.args or ())):
            raise SqlParseError(f"a window call must be a whole SELECT item: {_term_text(e)}")
        if spec is None:
            spec = e.over
        elif (e.over.partition_by, e.over.order_by) != (spec.partition_by, spec.order_by):
            raise SqlParseError("all window calls of a statement must share PARTITION BY and ORDER BY: "
                                f"({_window_text(e.over)}) differs from ({_window_text(spec)})")
        call = f"{e.name}({'*' if e.star else ', '.join(_expr_text(a) for a in (e.args or ()))})"
        kind = _WINDOW_KINDS.get(e.name.lower())
        if kind is None:
            raise SqlParseError(f"{e.name} is not a window function of this build")
        if e.args is None:
            raise SqlParseError(f"{e.name}(...) over: the arguments must be plain columns")
        alias = f.alias.value if isinstance(f, A.ExprWithAlias) else None
        name = alias if alias is not None else call.lower()
        if any(it.name == name for it in items):
            raise SqlParseError(f"two window calls would both be named {name!r}: give one an alias")
        frame = A.WindowFrame(e.over.frame)
        if e.star:
            if kind != A.WindowKind.COUNT:
                raise SqlParseError(f"{e.name}(*) is not a window function; only count(*) takes '*'")
            items.append(A.WindowItem(A.WindowKind.COUNT_STAR, name, None, frame))
        elif kind in (A.WindowKind.ROW_NUMBER, A.WindowKind.RANK, A.WindowKind.DENSE_RANK):
            if e.args:
                raise SqlParseError(f"{e.name} takes no argument: {call}")
            items.append(A.WindowItem(kind, name))
        elif kind in (A.WindowKind.LAG, A.WindowKind.LEAD):
            if len(e.args) not in (1, 2):
                raise SqlParseError(f"{e.name} takes a column and an optional offset: {call}")
            offset = 1
            if len(e.args) == 2:
                k = e.args[1]
                if not (isinstance(k, A.ValueExpr) and isinstance(k.value, A.Number) and k.value.text.isdigit()):
                    raise SqlParseError(f"the offset of {e.name} must be a non-negative integer literal: {call}")
                offset = int(k.value.text)
            items.append(A.WindowItem(kind, name, e.args[0], A.WindowFrame.PARTITION, offset))
        elif len(e.args) != 1:
            raise SqlParseError(f"{e.name} takes exactly one column: {call}")
        else:
            items.append(A.WindowItem(kind, name, e.args[0], frame))
        ident = A.Identifier(A.Ident(name))
        projection.append(A.ExprWithAlias(ident, f.alias) if isinstance(f, A.ExprWithAlias) else A.UnnamedExpr(ident))
    return tuple(spec.partition_by), tuple(spec.order_by), tuple(items), tuple(projection)


# ---- INNER JOIN: the ON condition as key pairs -------------------------------------------------------------
def join_plan(select: Select):
    """A `Select` with one `[inner] join ... on <cond>` -> the key pairs `((left column, right column), ...)` as
    `record_utils.join_records` takes them (None: the statement has no join).  `<cond>` must be a conjunction (AND,
    parentheses allowed) of `=` between one column qualified with the left table's alias and one qualified with the right
    table's alias, in either order; the pairs come out as (left, right)."""
    if not select.joins:
        return None
    if len(select.joins) != 1:
        raise SqlParseError(f"one JOIN per statement is supported, {len(select.joins)} are written")
    join = select.joins[0]
    la = select.from_.alias if select.from_ is not None else None
    ra = join.table.alias
    if la is None or ra is None:
        raise SqlParseError("both tables of a JOIN need an alias: the ON condition names its columns through them")
    if la == ra:
        raise SqlParseError(f"both tables of the JOIN have the alias {la!r}")

    def side(e: A.Expr) -> Optional[str]:
        if isinstance(e, A.CompoundIdentifier) and len(e.idents) == 2 and e.idents[0].value in (la, ra):
            return e.idents[0].value
        return None

    pairs: List[Tuple[A.Expr, A.Expr]] = []

    def walk(e: A.Expr) -> None:
        if isinstance(e, A.Nested):
            walk(e.expr)
        elif isinstance(e, A.BinaryOp) and e.op == A.BinaryOperator.And:
            walk(e.left)
            walk(e.right)
        elif isinstance(e, A.BinaryOp) and e.op == A.BinaryOperator.Eq and {side(e.left), side(e.right)} == {la, ra}:
            pairs.append((e.left, e.right) if side(e.left) == la else (e.right, e.left))
        else:
            raise SqlParseError(f"the ON condition of an INNER JOIN must be a conjunction of {la}.<column> = {ra}.<column>; "
                                f"found {_term_text(e)}")

    walk(join.on)
    return tuple(pairs)


def _term_text(e: A.Expr) -> str:
    if isinstance(e, A.Nested):
        return f"({_term_text(e.expr)})"
    if isinstance(e, A.BinaryOp):
        return f"{_term_text(e.left)} {e.op.value} {_term_text(e.right)}"
    if isinstance(e, A.ValueExpr):
        v = e.value
        return v.text if isinstance(v, A.Number) else repr(v.value) if hasattr(v, "value") else repr(v)
    return _expr_text(e)


def parse_expr(text: str) -> A.Expr:
    """Parse one SQL scalar expression (what follows WHERE, or one select item's expression)."""
    p = _Parser(_tokenize(text))
    e = p.parse_expr(0)
    if p.peek()[0] != "eof":
        raise SqlParseError(f"trailing tokens after expression: {p.peek()[1]!r}")
    return e


def parse_select(text: str) -> Select:
    p = _Parser(_tokenize(text))
    s = p.parse_select()
    if p.peek()[0] != "eof":
        raise SqlParseError(f"trailing tokens after statement: {p.peek()[1]!r}")
    return s


def parse_statements(text: str) -> List[Select]:
    """Split on ';' like the reference's multi-statement handling (planner/test_sqlparser_behavior.rs)."""
    toks = _tokenize(text)
    stmts, cur = [], []
    for t in toks:
        if t == ("op", ";"):
            if cur:
                stmts.append(cur)
            cur = []
        else:
            cur.append(t)
    if cur:
        stmts.append(cur)
    return [_Parser(s).parse_select() for s in stmts]
