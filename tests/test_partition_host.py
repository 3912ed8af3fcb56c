"""CPU: the hash partitioning's host side -- the pinned hash of include/chq.h restated by
tests/partition_reference.py and checked against the published pins, the properties of a partitioning, a balance bound that
guards against a degenerate hash, `repartition_records` between two ranks over gloo (with the reference as the
partitioning), and the argument errors of `partition_records` that need no GPU."""
import decimal
import os

import numpy as np
import pyarrow as pa
import pytest

import chapterhouseqe_amd as chq
from chapterhouseqe_amd import sqlast as A

from . import join_reference as J
from . import partition_reference as P
from . import sort_reference as R


def one_row(*arrays):
    return pa.RecordBatch.from_arrays(list(arrays), names=[f"k{i}" for i in range(len(arrays))])


def dec_bits(lo, hi):
    return pa.Array.from_buffers(pa.decimal128(38, 4), 1, [None, pa.py_buffer(np.array([lo, hi], dtype=np.uint64).tobytes())])


# (one-key rows unless said otherwise: the key columns, h, the partition id for P = 8)
PINS = [
    ("Int32 0", [pa.array([0], pa.int32())], 0x0092d4ed7de0c088, 0),
    ("Int32 1", [pa.array([1], pa.int32())], 0x94e150e41a43b226, 4),
    ("Int32 -1", [pa.array([-1], pa.int32())], 0xfe12a53901f3d298, 7),
    ("Int64 1", [pa.array([1], pa.int64())], 0x41409e06ef72b8dd, 2),
    ("Int8 1", [pa.array([1], pa.int8())], 0x9fef32a9e52a455e, 4),
    ("Float32 1.0", [pa.array([1.0], pa.float32())], 0x15337105b7991415, 0),
    ("Float64 -0.0", [pa.array([-0.0], pa.float64())], 0x2fcbb7fed7a3a57f, 1),
    ("Float64 +0.0", [pa.array([0.0], pa.float64())], 0x266f0d1be6fa9718, 1),
    ("Decimal128 lo = 1, hi = 0", [dec_bits(1, 0)], 0xad12674ac31d7352, 5),
    ("Utf8 ''", [pa.array([""])], 0x123cd2e5690c09b0, 0),
    ("Utf8 'a'", [pa.array(["a"])], 0x8fdebbde62f89937, 4),
    ("Utf8 'abcdefgh'", [pa.array(["abcdefgh"])], 0xca14c6926a818804, 6),
    ("Utf8 'abcdefghi'", [pa.array(["abcdefghi"])], 0x77b23fc57c99d85a, 3),
    ("null", [pa.array([None], pa.int32())], 0x3836f0681055a942, 1),
    ("(Int32 7, Utf8 'xy')", [pa.array([7], pa.int32()), pa.array(["xy"])], 0xc13e2af252d0d9ed, 6),
]


@pytest.mark.parametrize("name,arrays,h,pid", PINS, ids=[p[0] for p in PINS])
def test_pins(name, arrays, h, pid):
    rec = one_row(*arrays)
    assert int(P.row_hashes(rec, rec.schema.names)[0]) == h
    assert int(P.partition_ids(rec, rec.schema.names, 8)[0]) == pid
    parts = P.partition(rec, rec.schema.names, 8)
    assert [b.num_rows for b in parts] == [1 if p == pid else 0 for p in range(8)]


def test_pinned_ids_for_256_partitions_and_the_null_of_any_type():
    rec = one_row(pa.array([1], pa.int32()))
    assert int(P.partition_ids(rec, ["k0"], 256)[0]) == 148
    for t in (pa.int8(), pa.float64(), pa.utf8(), pa.bool_(), pa.decimal128(38, 4)):          # V(null) = 0 whatever the type
        assert int(P.row_hashes(one_row(pa.array([None], t)), ["k0"])[0]) == 0x3836f0681055a942
    assert int(P.fmix64(np.array([0], dtype=np.uint64))[0]) == 0


def test_a_boolean_is_one_byte_and_widths_hash_apart():
    t, i8 = one_row(pa.array([True])), one_row(pa.array([1], pa.int8()))
    assert P.row_hashes(t, ["k0"])[0] == P.row_hashes(i8, ["k0"])[0]          # one byte holding 1, L = 1: the same bits
    hs = {int(P.row_hashes(one_row(pa.array([5], ty)), ["k0"])[0]) for ty in (pa.int8(), pa.int16(), pa.int32(), pa.int64())}
    assert len(hs) == 4


def mixed_batch(rng, n):
    return pa.RecordBatch.from_arrays([
        pa.array(rng.integers(0, 40, n).astype(np.int32), mask=rng.random(n) < 0.15),
        pa.array([["", "a", "abcdefgh", "abcdefghi", "x" * 17][i] for i in rng.integers(0, 5, n)], mask=rng.random(n) < 0.15),
        pa.array(rng.choice([0.0, -0.0, np.nan, 1.0], n).astype(np.float64)),
        pa.array([decimal.Decimal(int(x)).scaleb(-2) for x in rng.integers(-5, 5, n)], type=pa.decimal128(20, 2)),
        pa.array(rng.random(n) < 0.5, mask=rng.random(n) < 0.15),
        pa.array(np.arange(n, dtype=np.int32))], names=["k", "s", "f", "d", "b", "row"])


@pytest.mark.parametrize("keys", [["k"], ["s"], ["f"], ["d"], ["b"], ["k", "s"], ["s", "k"], ["b", "d", "f"]])
def test_partition_properties(keys):
    rng = np.random.default_rng(len(keys) + len(keys[0]))
    rec = mixed_batch(rng, 3000)
    batches = [rec.slice(0, 1000), rec.slice(1000, 0), rec.slice(1000, 2000)]
    for n_parts in (1, 3, 8, 256):
        parts = P.partition(batches, keys, n_parts)
        assert len(parts) == n_parts and all(b.schema == rec.schema for b in parts)
        rows = [b.column(5).to_pylist() for b in parts]
        assert sorted(r for p in rows for r in p) == list(range(3000))          # every row exactly once
        assert all(p == sorted(p) for p in rows)                                # input order kept
        home = {}
        for p, b in enumerate(parts):                                           # equal keys stay together
            for key in zip(*[J.key_bits(b.column(b.schema.get_field_index(k))) for k in keys]):          # (None: a null)
                assert home.setdefault(key, p) == p
        if n_parts > 1 and len(keys) == 1:
            assert sum(1 for p in rows if p) > 1                                # (no case passes vacuously)
    ids = P.partition_ids(rec, keys, 8)
    assert np.array_equal(ids, P.partition_ids(rec, keys, 8))
    if keys == ["k"]:                                                           # the null row is as pinned
        nulls = np.flatnonzero(~np.asarray(rec.column(0).is_valid()))
        assert len(nulls) and set(ids[nulls].tolist()) == {1}
    if len(keys) == 2:                                                          # the order of the keys matters
        assert not np.array_equal(P.row_hashes(rec, keys), P.row_hashes(rec, keys[::-1]))


def test_minus_zero_and_nan_payloads_are_taken_by_bits():
    bits = np.array([0x0000000000000000, 0x8000000000000000, 0x7ff8000000000001, 0x7ff8000000000002], dtype=np.uint64)
    rec = one_row(pa.array(bits.view(np.float64)))
    assert len(set(P.row_hashes(rec, ["k0"]).tolist())) == 4


def test_balance_of_65536_consecutive_int32_keys_over_8_partitions():
    """guards against a degenerate hash; not a tuning target"""
    n, n_parts = 65536, 8
    rec = one_row(pa.array(np.arange(n, dtype=np.int32)))
    counts = np.bincount(P.partition_ids(rec, ["k0"], n_parts), minlength=n_parts)
    print("rows per partition:", counts.tolist())
    assert counts.sum() == n
    assert all(0.9 * n / n_parts <= c <= 1.1 * n / n_parts for c in counts), counts.tolist()


# ---------------------------------------------------------------------------------------------- world_size 2 (gloo)
def _tables():
    rng = np.random.default_rng(17)

    def side(n, row_name, extra):
        return pa.RecordBatch.from_arrays([
            pa.array(rng.integers(0, 60, n).astype(np.int32), mask=rng.random(n) < 0.15),
            pa.array(np.arange(n, dtype=np.int32)),
            pa.array([f"{extra}{i % 11}" for i in range(n)], mask=rng.random(n) < 0.2)], names=["k", row_name, extra])

    left, right = side(600, "lrow", "ltag"), side(400, "rrow", "rtag")
    cut = lambda b, step: [b.slice(o, min(step, b.num_rows - o)) for o in range(0, b.num_rows, step)]   # noqa: E731
    return cut(left, 100), cut(right, 70)


def _row_multiset(batches):
    rows = []
    for b in batches:
        rows += list(zip(*[c.to_pylist() for c in b.columns])) if b.num_columns else []
    return sorted(rows, key=repr)


def _write(path, batches):
    with pa.OSFile(path, "wb") as f, pa.ipc.new_file(f, batches[0].schema) as w:
        for b in batches:
            w.write_batch(b)


def _read(path):
    return pa.ipc.open_file(path).read_all().to_batches()


def _repartition_worker(rank, world, port, tmpdir):
    import torch.distributed as dist
    from chapterhouseqe_amd.operators.distributed import repartition_records, shard_record_ids
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    try:
        left, right = _tables()                                        # every rank regenerates the same tables
        keys = P.to_plan(["k"])

        def ref(records, aliases, key_exprs, n):
            return P.partition(records, P.from_plan(key_exprs), n)

        owned = {}
        for name, batches in (("left", left), ("right", right)):
            mine = [batches[i] for i in shard_record_ids(range(len(batches)), rank, world)]
            got = repartition_records(mine, [[] for _ in range(3)], keys, partition_fn=ref)
            assert len(got) == world and all(g.schema == batches[0].schema for g in got)
            # ordered by source rank: part `rank` of what source rank q held, rows in q's input order
            for q, g in enumerate(got):
                theirs = [batches[i] for i in shard_record_ids(range(len(batches)), q, world)]
                assert g.equals(P.partition(theirs, ["k"], world)[rank]), (name, q)
            owned[name] = got
            _write(os.path.join(tmpdir, f"{name}{rank}.arrow"), got)
        _write(os.path.join(tmpdir, f"joined{rank}.arrow"), [J.join(owned["left"], owned["right"], [("k", "k")])[2]])
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_repartition_between_two_ranks_over_gloo(tmp_path):
    import socket
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    world = 2
    mp.spawn(_repartition_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    left, right = _tables()
    for name, whole in (("left", left), ("right", right)):
        per_rank = [_read(str(tmp_path / f"{name}{r}.arrow")) for r in range(world)]
        assert _row_multiset([b for rank in per_rank for b in rank]) == _row_multiset(whole)          # the union is the input
        key_sets = [{k for b in rank for k in J.key_bits(b.column(0))} for rank in per_rank]
        assert all(len(s) > 5 for s in key_sets) and not (key_sets[0] & key_sets[1])                   # disjoint key sets
    joined = [_read(str(tmp_path / f"joined{r}.arrow")) for r in range(world)]
    exp = J.join(left, right, [("k", "k")])[2]
    assert exp.num_rows > 1000 and all(sum(b.num_rows for b in j) > 100 for j in joined)
    assert _row_multiset([b for j in joined for b in j]) == _row_multiset([exp])


def test_repartition_with_one_rank_needs_no_process_group():
    from chapterhouseqe_amd.operators.distributed import repartition_records
    left, _ = _tables()
    got = repartition_records(left, [[]] * 3, P.to_plan(["k"]), partition_fn=lambda recs, al, keys, n: P.partition(recs, P.from_plan(keys), n))
    assert len(got) == 1 and got[0].equals(R.join(left))
    with pytest.raises(ValueError):
        repartition_records(left, [[]] * 3, P.to_plan(["k"]), partition_fn=lambda recs, al, keys, n: [])


# ---------------------------------------------------------------------------------------------- arguments
def test_partition_records_argument_errors_that_need_no_gpu():
    rec = mixed_batch(np.random.default_rng(0), 10)
    al = [[] for _ in range(rec.num_columns)]
    k = [A.ident("k")]
    with pytest.raises(ValueError):
        chq.partition_records([], al, k, 8)
    for bad in ("8", 8.0, None, True):
        with pytest.raises(TypeError):
            chq.partition_records(rec, al, k, bad)
    with pytest.raises(TypeError):
        chq.partition_records(rec, al, ["k"], 8)                       # a key is an expression, not a name
    other = pa.RecordBatch.from_arrays([pa.array([1, 2], type=pa.int64())], names=["k"])
    with pytest.raises(chq.ChqError) as ei:
        chq.partition_records([rec, other], al, k, 8)
    assert ei.value.code == 22
    assert "partition_records" in chq.__all__
