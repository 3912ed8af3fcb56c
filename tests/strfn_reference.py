"""The tests' reference for the scalar string functions (include/chq.h: chq_expr_function, CHQ_BINOP_STRING_CONCAT): a plain
Python restatement of the rules on `bytes`.  Everything is bytewise; case and whitespace are ASCII only; a code point start is a
byte that is not 0x80..0xBF.  tests/test_strfn_host.py pins it to sqlite3 and pyarrow.compute on valid UTF-8."""
import random


def is_start(b: int) -> bool:
    return not (0x80 <= b <= 0xBF)


def upper(s: bytes) -> bytes:
    return bytes(b - 32 if 0x61 <= b <= 0x7A else b for b in s)


def lower(s: bytes) -> bytes:
    return bytes(b + 32 if 0x41 <= b <= 0x5A else b for b in s)


def length(s: bytes) -> int:
    return sum(1 for b in s if is_start(b))


def octet_length(s: bytes) -> int:
    return len(s)


def substring(s: bytes, p: int, n=None) -> bytes:
    """positions are 1-based code points; q is kept iff p <= q, q < p + n (with n) and 1 <= q <= length(s)"""
    assert n is None or n >= 0
    starts = [i for i, b in enumerate(s) if is_start(b)]

    def kth(k):   # byte index of the k-th start (k >= 1), or the row's end
        return starts[k - 1] if k <= len(starts) else len(s)
    first = 0 if p <= 1 else kth(p)
    end = len(s) if n is None else kth(max(p + n, 1))
    return s[first:end]


def trim(s: bytes) -> bytes:
    return s.strip(b" ")


def ltrim(s: bytes) -> bytes:
    return s.lstrip(b" ")


def rtrim(s: bytes) -> bytes:
    return s.rstrip(b" ")


def concat(*parts):
    return None if any(p is None for p in parts) else b"".join(parts)


UNARY = {"upper": upper, "lower": lower, "length": length, "char_length": length, "character_length": length, "octet_length": octet_length,
         "trim": trim, "ltrim": ltrim, "rtrim": rtrim}


def over(fn, values, *args):
    """fn over a list of bytes / None, null where the input is"""
    return [None if v is None else fn(v, *args) for v in values]


def sql_quote(s: str) -> str:
    return "'" + s.replace("'", "''") + "'"


def substring_sql(operand: str, p: int, n=None, comma=False, name="substring") -> str:
    if comma or name != "substring":
        return f"{name}({operand}, {p}" + ("" if n is None else f", {n}") + ")"
    return f"substring({operand} from {p}" + ("" if n is None else f" for {n}") + ")"


# valid UTF-8 with 1- to 4-byte code points, spaces, tabs, empties
CORNERS = ["", " ", "  ", "a", "Z", "abc", "ABC", "aBc", " a ", "  ab  ", "a b", " \t a \t ", "\ta\t", "é", "É", "héllo", "日本語", "a日b", "😀", "a😀é日 ",
           "zZ@[`{", "az AZ", "  ", "x" * 17, " " * 5 + "é" + " " * 3, "ß", "ÀÉ", "'q'"]
# invalid UTF-8: leading continuation bytes, a truncated 4-byte sequence at the end, lone 0xFF (and mixes)
INVALID = [b"\x80", b"\x80\x80a", b"\xbf\xbfab\x80", b"ab\xf0\x9f\x98", b"\xf0\x9f", b"\xff", b"a\xffb", b"\xff\xff", b"\x80 a \x80", b" \xf0\x9f\x98",
           b"\xc3", b"a\xc3", b"\x80\xc3\xa9\x80b", b"\xe6\x97", b"A\x80z\xbf"]
WINDOWS = [(p, n) for p in (-3, -1, 0, 1, 2, 3, 5, 6, 7, 100) for n in (None, 0, 1, 2, 3, 100)]


def random_strings(count=600, seed=20261020):
    rng = random.Random(seed)
    alphabet = ["a", "Z", "m", "é", "日", "😀", " ", " ", "\t", "Q"]
    return ["".join(rng.choice(alphabet) for _ in range(rng.randint(0, 9))) for _ in range(count)]
