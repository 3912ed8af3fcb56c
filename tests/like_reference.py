"""Reference of the LIKE and IS [NOT] NULL predicates for the tests (tests only; the product never imports it).

`like(s, pattern, escape)` restates SQL LIKE as a regular expression on `str`: `%` = any run of characters (`.*`), `_` = one
character (`.`, one code point: a `str` is a sequence of code points), `escape` followed by any character = that character,
everything else itself; `re.fullmatch` with `re.S` so that `.` takes a newline.  There is NO default escape character.  On
valid UTF-8 "any run of bytes" and "any run of characters" are the same thing, because every other element of a pattern is
made of whole characters."""
from __future__ import annotations

import re
from typing import List, Optional, Sequence

import pyarrow as pa

PATTERNS = ["", "%", "%%", "_", "__%", "%_", "_%_", "a%", "%a", "%a%", "a%b", "a%b%c", "%aab%", "%ab%ab%"]
# the fixed table: the patterns above against these (among them `%aab%` against `aaab`, `%ab%ab%` against `abab` and `abaab`), and the multibyte /
# newline / escape corners as (string, pattern, escape)
STRINGS = ["", "a", "b", "ab", "ba", "aa", "abc", "aXb", "abXc", "aaab", "abab", "abaab", "aab", "xaaby", "a\nb", "\n", "é", "aé", "éa",
           "héllo", "日本語", "ab%", "a_b", "%", "_"]
EXTRA = [("héllo", "h_llo", None), ("héllo", "h__llo", None), ("héllo", "_____", None), ("héllo", "______", None), ("日本語", "___", None),
         ("日本語", "_本_", None), ("日本語", "%本%", None), ("é", "_", None), ("é", "__", None), ("aé", "a_", None), ("éa", "_a", None),
         ("a\nb", "a_b", None), ("a\nb", "a%b", None), ("a\nb", "a%", None), ("\n", "_", None), ("\n\n", "%\n", None),
         ("50%", "50!%", "!"), ("50x", "50!%", "!"), ("a_b", "a!_b", "!"), ("axb", "a!_b", "!"), ("a!b", "a!!b", "!"), ("a!b", "a!!_", "!"),
         ("ab", "!a!b", "!"), ("100%", "%!%", "!"), ("100%x", "%!%", "!"), ("%", "%%", "%"), ("a", "%%", "%"), ("_", "__", "_"),
         ("x", "__", "_"), ("a\\b", "a\\b", None), ("a\\%", "a\\%", None), ("a\\xyz", "a\\%", None), ("a%", "a\\%", "\\"),
         ("aaab", "%aab%", None), ("abab", "%ab%ab%", None), ("abaab", "%ab%ab%", None), ("aba", "%ab%ab%", None)]


class TrailingEscape(ValueError):
    """the pattern ends in a lone escape character"""


def to_regex(pattern: str, escape: Optional[str] = None) -> str:
    out, i = [], 0
    while i < len(pattern):
        c = pattern[i]
        if escape is not None and c == escape:
            if i + 1 >= len(pattern):
                raise TrailingEscape(pattern)
            out.append(re.escape(pattern[i + 1]))
            i += 2
            continue
        out.append(".*" if c == "%" else "." if c == "_" else re.escape(c))
        i += 1
    return "".join(out)


def like(s: str, pattern: str, escape: Optional[str] = None) -> bool:
    return re.fullmatch(to_regex(pattern, escape), s, re.S) is not None


def is_null(v, negated: bool = False) -> bool:
    return (v is None) != negated


def like_values(values: Sequence[Optional[str]], pattern: str, escape: Optional[str] = None, negated: bool = False) -> List[Optional[bool]]:
    rx = re.compile(to_regex(pattern, escape), re.S)
    return [None if v is None else ((rx.fullmatch(v) is not None) != negated) for v in values]


def like_array(arr: pa.Array, pattern: str, escape: Optional[str] = None, negated: bool = False) -> pa.Array:
    """a pyarrow Utf8 array -> Boolean, null exactly where the input is null"""
    return pa.array(like_values(arr.to_pylist(), pattern, escape, negated), type=pa.bool_())


def is_null_array(arr: pa.Array, negated: bool = False) -> pa.Array:
    """any pyarrow array -> Boolean without nulls"""
    return pa.array([is_null(None if not ok else 0, negated) for ok in arr.is_valid().to_pylist()], type=pa.bool_())


def arrow_pattern(pattern: str, escape: Optional[str]) -> Optional[str]:
    """the same pattern for pyarrow.compute.match_like, whose escape is always the backslash; None when the pattern holds a
    backslash that is not our escape (it would mean something else there)"""
    out, i = [], 0
    while i < len(pattern):
        c = pattern[i]
        if escape is not None and c == escape:
            if i + 1 >= len(pattern):
                raise TrailingEscape(pattern)
            nxt = pattern[i + 1]   # (match_like's backslash escapes `%`, `_` and itself only)
            out.append("\\" + nxt if nxt in "%_\\" else nxt)
            i += 2
            continue
        if c == "\\":
            return None
        out.append(c)
        i += 1
    return "".join(out)


def sql_quote(s: str) -> str:
    return "'" + s.replace("'", "''") + "'"


def like_sql(operand: str, pattern: str, escape: Optional[str] = None, negated: bool = False) -> str:
    return f"{operand} {'not ' if negated else ''}like {sql_quote(pattern)}" + (f" escape {sql_quote(escape)}" if escape is not None else "")
