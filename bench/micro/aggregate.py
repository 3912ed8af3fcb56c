"""GROUP BY throughput: chq.aggregate_record on a device-resident batch of the reference's sample
shape (id: Int32, value1: Utf8 of 8 letters, value2: Float32; create_sample_data.rs) plus `bucket` = id % 1000 materialised
as an Int32 column, against torch on the same device -- stable torch.sort of the key, unique_consecutive for the group
sizes, segment_reduce for the aggregates -- timed alternately in one process.

  group by bucket: sum(value2), count(*)        100 M rows, 1000 groups
  group by value1: count(*)                     100 M rows, 8-letter strings: almost every row a group of its own
  no key: sum(value2), min(value2), max(value2) 100 M rows, one group

Times are steady state (one warm-up call per query): `call` is the host clock around the call, which ends in a stream
synchronisation; `kernels` is the library's own event pair around its launches (context option time_kernels), the sort
included.  `alg GB` is the bytes the library's pass structure reads and writes (chq_call_stats); `of peak` = those bytes at
8 TB/s over the kernel time.  torch's keys are prepared outside the timing; its sums are Float32 accumulations where the
library's are Float64.
usage: python bench/micro/aggregate.py [--rows N] [--reps R] [--json PATH]"""
import argparse
import json
import sys
import time

sys.path.insert(0, ".")
import chapterhouseqe_amd as chq   # noqa: E402
from chapterhouseqe_amd import sqlast as A   # noqa: E402

PEAK = 8.0e12

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=100_000_000)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--json", default=None)
args = ap.parse_args()

import torch   # noqa: E402

dev = torch.device("cuda", 0)
ctx = chq.Context(0)
ctx.set_option("time_kernels", 1)
results = []

n = args.rows
g = torch.Generator(device=dev).manual_seed(0)
ids = torch.arange(n, dtype=torch.int32, device=dev)
bucket = ids % 1000
letters = torch.randint(ord("a"), ord("z") + 1, (n, 8), dtype=torch.uint8, device=dev, generator=g)
offs = torch.arange(n + 1, dtype=torch.int32, device=dev) * 8
v2 = torch.rand(n, device=dev, generator=g) * 100
torch.cuda.synchronize()
rec = chq.DeviceRecordBatch.from_device_pointers(
    [("id", "i", ids.data_ptr()), ("value1", "u", offs.data_ptr(), letters.data_ptr()), ("value2", "f", v2.data_ptr()),
     ("bucket", "i", bucket.data_ptr())], n, ctx=ctx, keepalive=[ids, letters, offs, v2, bucket])
ALIASES = [[]] * 4


def be_key(x8):
    """the 8 letters as one int64 whose signed order is their byte order (torch has no unsigned 64-bit sort)"""
    x = x8.to(torch.int64)
    k = torch.zeros(x8.shape[0], dtype=torch.int64, device=dev)
    for b in range(8):
        k = (k << 8) | x[:, b]
    return k ^ (-(1 << 63))


v1_key = be_key(letters)
torch.cuda.synchronize()


def time_chq(keys, items):
    best, kernels, stats = 1e9, 1e9, None
    chq.aggregate_record(rec, ALIASES, keys, items, ctx=ctx).release()   # warm-up
    for _ in range(args.reps):
        t0 = time.perf_counter()
        out = chq.aggregate_record(rec, ALIASES, keys, items, ctx=ctx)
        dt = time.perf_counter() - t0
        stats = ctx.last_stats()
        out.release()
        best = min(best, dt)
        kernels = min(kernels, stats["kernel_ns"] * 1e-9)
    return best, kernels, stats


def time_torch(fn):
    try:
        fn()
    except RuntimeError as err:   # an operator this torch build lacks on the device: report the library's side alone
        print(f"torch side failed: {err}", flush=True)
        return None
    torch.cuda.synchronize()
    best = 1e9
    for _ in range(args.reps):
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        out = fn()
        e.record()
        torch.cuda.synchronize()
        best = min(best, s.elapsed_time(e) * 1e-3)
        del out
    return best


def report(name, chq_t, torch_t):
    call, kern, st = chq_t
    alg = st["bytes_read_alg"] + st["bytes_written_alg"]
    row = {"case": name, "rows": n, "groups": st["rows_out"], "chq_call_ms": call * 1e3, "chq_kernels_ms": kern * 1e3,
           "chq_rows_per_s": n / call, "alg_gb": alg / 1e9, "of_peak": alg / PEAK / kern if kern > 0 else None,
           "launches": st["launches"], "torch_ms": torch_t * 1e3 if torch_t else None,
           "chq_kernels_over_torch": kern / torch_t if torch_t else None}
    results.append(row)
    torch_text = f"torch {torch_t * 1e3:8.1f} ms | chq / torch {kern / torch_t:.2f}" if torch_t else "torch: not measured"
    print(f"{name:44s} {n / 1e6:5.0f} M rows -> {st['rows_out']:>9d} groups: chq call {call * 1e3:8.1f} ms, kernels {kern * 1e3:8.1f} ms, "
          f"{alg / 1e9:6.1f} alg GB = {100 * alg / PEAK / kern:4.1f} % of 8 TB/s, {st['launches']} launches | {torch_text}", flush=True)


def torch_grouped(key, reduces):
    """stable sort of the key, run lengths, one segment_reduce per aggregate over the permuted values"""
    skey, perm = torch.sort(key, stable=True)
    uniq, counts = torch.unique_consecutive(skey, return_counts=True)
    outs = [uniq, counts]
    for values, how in reduces:
        outs.append(torch.segment_reduce(values.index_select(0, perm), how, lengths=counts))
    return outs


def item(kind, name, col=None, key_index=-1):
    return A.AggItem(kind, name, key_index, A.ident(col) if col else None)


K = A.AggKind
cases = [
    ("group by bucket: sum(value2), count(*)", [A.ident("bucket")],
     [item(K.KEY, "bucket", key_index=0), item(K.SUM, "sum(value2)", "value2"), item(K.COUNT_STAR, "count(*)")],
     lambda: torch_grouped(bucket, [(v2, "sum")])),
    ("group by value1: count(*)", [A.ident("value1")], [item(K.KEY, "value1", key_index=0), item(K.COUNT_STAR, "count(*)")],
     lambda: torch_grouped(v1_key, [])),
    ("no key: sum, min, max of value2", [],
     [item(K.SUM, "sum(value2)", "value2"), item(K.MIN, "min(value2)", "value2"), item(K.MAX, "max(value2)", "value2")],
     lambda: (v2.sum(), v2.min(), v2.max())),
]
for name, keys, items, tfn in cases:
    c = time_chq(keys, items)      # alternate: ours, then torch's, query by query
    t = time_torch(tfn)
    report(name, c, t)
rec.release()

if args.json:
    with open(args.json, "w") as fh:
        json.dump(results, fh, indent=1)
