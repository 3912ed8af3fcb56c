"""Host: the Utf8 reference (utf8_reference.py) against pyarrow and the CPU oracle, and the conditions on its generated inputs
that the GPU tests rely on -- every profile on its declared side of the column rule, the group24 groups and the runs3088 runs
holding exactly the byte counts they are named for."""
import numpy as np
import pyarrow as pa
import pytest

from chapterhouseqe_amd import sqlast as A
from oracle import oracle as O

from . import utf8_reference as R

N = 4200


def test_every_byte_names_its_place():
    lengths = R.LENGTH_PROFILES["cycle41"].lengths(300)
    arr = R.make_utf8(lengths, lead=5)
    offsets, data, valid = R.utf8_parts(arr)
    assert offsets[0] == 5 and bytes(data[:5]) == b"     " and valid.all() and arr.null_count == 0
    for r in (0, 1, 40, 41, 299):
        want = bytes(0x21 + (r * 131 + k * 7) % 94 for k in range(int(lengths[r])))
        assert bytes(data[offsets[r]:offsets[r + 1]]) == want and arr[r].as_py() == want.decode()
    rows = arr.to_pylist()
    assert all(rows[r][:16] != rows[r + 1][:16] for r in range(16, 40))                      # neighbouring rows differ,
    assert all(rows[40][k:k + 4] != rows[40][k + 4:k + 8] for k in range(0, 32, 4))          # and neighbouring chunks of a row
    assert rows[40][:16] != rows[40][16:32]
    empty = R.make_utf8(np.zeros(7, dtype=np.int64))
    assert empty.buffers()[2].size == 0 and empty.to_pylist() == [""] * 7


@pytest.mark.parametrize("profile", list(R.LENGTH_PROFILES))
def test_expected_filter_is_arrow_filter(profile):
    lengths = R.LENGTH_PROFILES[profile].lengths(N)
    valid = np.random.default_rng(3).random(N) >= 0.2
    plain, nulls = R.make_utf8(lengths, lead=3), R.make_utf8(lengths, valid=valid)
    for name, sel in R.SELECTIONS.items():
        keep = sel(N)
        assert keep.dtype == bool and keep.shape == (N,), name
        for arr in (plain, nulls, nulls.slice(65, N - 130)):
            k = keep[:len(arr)]
            offsets, data, ok = R.expected_filter(arr, k)
            want = arr.filter(pa.array(k))
            assert offsets[0] == 0 and len(offsets) == len(want) + 1 and len(data) == offsets[-1], (profile, name)
            got = [bytes(data[offsets[i]:offsets[i + 1]]).decode() if ok[i] else None for i in range(len(want))]
            assert got == want.to_pylist(), (profile, name)
            assert int((~ok).sum()) == want.null_count, (profile, name)


def test_selections_are_what_their_names_say():
    n = R.N_GPU
    per_group = lambda keep: np.add.reduceat(keep.astype(np.int64), np.arange(0, n, 64))[:n // 64]
    assert not R.SELECTIONS["none"](n).any() and R.SELECTIONS["all"](n).all()
    for c in (1, 8, 15, 16, 17, 63):
        assert (per_group(R.SELECTIONS[f"count{c}"](n)) == c).all() and (per_group(R.SELECTIONS[f"scatter{c}"](n)) == c).all()
    assert not np.array_equal(R.SELECTIONS["count17"](n), R.SELECTIONS["scatter17"](n))
    for k, runs, rows in ((3, 16, 48), (4, 13, 52), (5, 11, 54)):   # utf8_copy_kernel: runs x 4 > rows -> row by row
        keep = R.SELECTIONS[f"runs{k}"](n)
        starts = keep & ~(np.concatenate([[False], keep[:-1]]) & (np.arange(n) % 64 != 0))   # (the kernel counts runs per group)
        assert (per_group(keep) == rows).all() and (per_group(starts) == runs).all()
        assert (runs * 4 > rows) == (k == 3)
    off = R.SELECTIONS["tiles_off"](n)
    assert not off[:R.TILE].any() and off[R.TILE:2 * R.TILE].all() and not off[2 * R.TILE:3 * R.TILE].any() and off[3 * R.TILE:].all()
    assert np.flatnonzero(R.SELECTIONS["first_and_last_row"](n)).tolist() == [0, n - 1]
    for p in (0.02, 0.5, 0.98):
        assert abs(R.SELECTIONS["random%02d" % round(p * 100)](n).mean() - p) < 0.01


@pytest.mark.parametrize("n", [R.N_GPU, N])
def test_profiles_lie_on_their_side_of_the_column_rule(n):
    for name, prof in R.LENGTH_PROFILES.items():
        lengths = prof.lengths(n)
        assert len(lengths) == n and (lengths >= 0).all(), name
        if n == N and name.startswith("spike"):
            continue   # (three 70 000-byte rows outweigh 4200 rows: the side is declared for the GPU tests' row count)
        assert (int(lengths.sum()) <= 24 * n) == (prof.side == "short"), (name, int(lengths.sum()), 24 * n)
    for a, b in (("group24_short", "group24_long"),):   # once to each side, as close as one group
        assert 0 < 24 * n - int(R.LENGTH_PROFILES[a].lengths(n).sum()) < 24 * 64
        assert 0 < int(R.LENGTH_PROFILES[b].lengths(n).sum()) - 24 * n < n // 64
        if n == R.N_GPU:   # (the figures of DESIGN.md's threshold table)
            assert 24 * n - int(R.LENGTH_PROFILES[a].lengths(n).sum()) == 1151 and int(R.LENGTH_PROFILES[b].lengths(n).sum()) - 24 * n == 385


def _group_bytes(lengths, keep):
    n = len(lengths) // 64 * 64
    return (lengths[:n] * keep[:n]).reshape(-1, 64).sum(axis=1)


def test_group24_groups_hold_24_bytes_per_row_and_one_more():
    n = R.N_GPU
    for name in ("group24_short", "group24_long"):
        lengths = R.LENGTH_PROFILES[name].lengths(n)
        gb = _group_bytes(lengths, np.ones(n, dtype=bool))
        first = 2 if name == "group24_short" else 0
        assert (gb[first::2] == R.GROUP24_EVEN).all() and (gb[1::2] == R.GROUP24_ODD).all()
        assert R.GROUP24_EVEN == 24 * 64 and R.GROUP24_ODD == 24 * 64 + 1
        per_group = lengths[:n // 64 * 64].reshape(-1, 64)
        assert (per_group[first:].min(axis=1) < per_group[first:].max(axis=1)).all()   # unequal lengths inside every group
        assert ((per_group[1::2] == 25).sum(axis=1) == 1).all()


def test_runs3088_runs_hold_their_byte_counts():
    n = R.N_GPU
    # `all`: one run per group
    lengths = R.LENGTH_PROFILES["runs3088_all"].lengths(n)
    gb = _group_bytes(lengths, R.SELECTIONS["all"](n))
    assert gb.tolist() == [R.RUN_TARGETS[g % 10] for g in range(len(gb))] and len(gb) > 10
    # `runs4`: lanes 5 j .. 5 j + 3 of every 16th group
    lengths = R.LENGTH_PROFILES["runs3088_runs4"].lengths(n)
    keep = R.SELECTIONS["runs4"](n)
    seen = set()
    for g in range(0, n // 64, R.RUNS4_GROUP_STRIDE):
        for j in range(13):
            rows = np.arange(64 * g + 5 * j, 64 * g + 5 * j + 4)
            assert keep[rows].all() and (j == 12 or not keep[rows[-1] + 1])
            want = R.RUN_TARGETS[(g // R.RUNS4_GROUP_STRIDE + j) % 10]
            assert int(lengths[rows].sum()) == want
            seen.add(want)
    assert seen == set(R.RUN_TARGETS)
    # the loop bounds of utf8_copy_kernel these straddle: lane 0 takes the four-chunk step from 3088 bytes, a second one from 7184
    assert {3087, 3088, 3089, 4095, 4096, 4097, 1023, 1024, 1025} < set(R.RUN_TARGETS) and max(R.RUN_TARGETS) >= 4096 + 3088 + 1008


# ---- comparisons ---------------------------------------------------------------------------------------------------------
def _oracle_or_none(rec, expr):
    try:
        return O.compute_value(rec, [[], []], expr)[0].to_pylist()
    except O.OracleError:
        return None


def _cmp(op, left, right):
    return A.BinaryOp(left, A.BinaryOperator[op], right)


def test_compare_bytes_is_the_oracles_comparison():
    t = len(R.COMPARE_TABLE)
    av, bv = R.compare_pairs(t * t)
    assert len(set(zip(av, bv))) == t * t
    checked = 0
    for with_nulls in (False, True):
        a = [None if with_nulls and i % 7 == 3 else v for i, v in enumerate(av)]
        b = [None if with_nulls and i % 5 == 1 else v for i, v in enumerate(bv)]
        rec = pa.RecordBatch.from_arrays([R.binary_column(a), R.binary_column(b, lead=3)], names=["a", "b"])
        for op in R.COMPARE_OPS:
            got = _oracle_or_none(rec, _cmp(op, A.ident("a"), A.ident("b")))
            if got is not None:
                assert got == [R.compare_bytes(op, x, y) for x, y in zip(a, b)], op
                checked += 1
            for lit in R.COMPARE_TABLE:
                if not R.is_utf8(lit):
                    continue
                node = A.string(lit.decode())
                got = _oracle_or_none(rec, _cmp(op, A.ident("a"), node))
                if got is not None:
                    assert got == [R.compare_bytes(op, x, lit) for x in a], (op, lit)
                    checked += 1
                got = _oracle_or_none(rec, _cmp(op, node, A.ident("a")))
                if got is not None:
                    assert got == [R.compare_bytes(op, lit, x) for x in a], (op, lit)
                    checked += 1
    # the oracle accepts every form, the columns that are not UTF-8 included: 2 null variants x 6 operators x (column against
    # column + 16 UTF-8 literals on either side)
    literals = sum(R.is_utf8(v) for v in R.COMPARE_TABLE)
    assert literals == 16 and checked == 2 * 6 * (1 + 2 * literals)
    assert R.compare_bytes("Lt", b"\x7f", b"\x80") and R.compare_bytes("Lt", b"a", b"a\x00") and R.compare_bytes("Lt", b"", b"\x00")
    assert R.compare_bytes("Eq", None, b"") is None and R.compare_bytes("Gt", b"", None) is None
