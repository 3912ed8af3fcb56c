"""AVG and COUNT(DISTINCT) throughput: chq.aggregate_record on the device-resident batch of
bench/micro/aggregate.py -- the reference's sample shape (id: Int32, value1: Utf8 of 8 letters, value2: Float32) plus
`bucket` = id % 1000 as an Int32 column.

  group by bucket: avg(value2)                    beside  group by bucket: sum(value2), count(value2)
  group by bucket: count(distinct id)             one more sort (bucket, id) and one more run finding; 1000 groups
  no key: count(distinct value1)                  the sort of the strings and a run finding; one group
  base: the three queries of bench/micro/aggregate.py, which use none of the new kinds -- run with --base-only against a
        library built from the parent commit (CHQ_LIB_PATH) and against this one in the same session, they say what the
        added instantiations of the reduce kernels cost the existing items

Times are steady state (one warm-up call per query) and MEDIANS of --reps calls: `call` is the host clock around the call,
which ends in a stream synchronisation; `kernels` is the library's own event pair around its launches (context option
time_kernels), the sorts included; `min` / `max` of the kernel time are that run's own spread.  `alg GB` is the bytes the
library's pass structure reads and writes and `launches` its kernel launches (chq_call_stats).
usage: python bench/micro/aggregate_ext.py [--rows N] [--reps R] [--base-only] [--json PATH]"""
import argparse
import json
import statistics
import sys
import time

sys.path.insert(0, ".")
import chapterhouseqe_amd as chq   # noqa: E402
from chapterhouseqe_amd import sqlast as A   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=100_000_000)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--base-only", action="store_true")
ap.add_argument("--json", default=None)
args = ap.parse_args()

import torch   # noqa: E402

dev = torch.device("cuda", 0)
ctx = chq.Context(0)
ctx.set_option("time_kernels", 1)

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


def item(kind, name, col=None, key_index=-1):
    return A.AggItem(kind, name, key_index, A.ident(col) if col else None)


K = A.AggKind
BUCKET = item(K.KEY, "bucket", key_index=0)
base = [
    ("base: group by bucket: sum(value2), count(*)", [A.ident("bucket")], [BUCKET, item(K.SUM, "sum(value2)", "value2"), item(K.COUNT_STAR, "count(*)")]),
    ("base: group by value1: count(*)", [A.ident("value1")], [item(K.KEY, "value1", key_index=0), item(K.COUNT_STAR, "count(*)")]),
    ("base: no key: sum, min, max of value2", [],
     [item(K.SUM, "sum(value2)", "value2"), item(K.MIN, "min(value2)", "value2"), item(K.MAX, "max(value2)", "value2")]),
]
new = [] if args.base_only else [
    ("group by bucket: sum(value2), count(value2)", [A.ident("bucket")],
     [BUCKET, item(K.SUM, "sum(value2)", "value2"), item(K.COUNT, "count(value2)", "value2")]),
    ("group by bucket: avg(value2)", [A.ident("bucket")], [BUCKET, item(K.AVG, "avg(value2)", "value2")]),
    ("group by bucket: count(distinct id)", [A.ident("bucket")], [BUCKET, item(K.COUNT_DISTINCT, "count(distinct id)", "id")]),
    ("no key: count(distinct value1)", [], [item(K.COUNT_DISTINCT, "count(distinct value1)", "value1")]),
]

results = []
for name, keys, items in base + new:
    chq.aggregate_record(rec, ALIASES, keys, items, ctx=ctx).release()   # warm-up
    calls, kernels, stats = [], [], None
    for _ in range(args.reps):
        t0 = time.perf_counter()
        out = chq.aggregate_record(rec, ALIASES, keys, items, ctx=ctx)
        calls.append(time.perf_counter() - t0)
        stats = ctx.last_stats()
        out.release()
        kernels.append(stats["kernel_ns"] * 1e-9)
    alg = stats["bytes_read_alg"] + stats["bytes_written_alg"]
    row = {"case": name, "rows": n, "groups": stats["rows_out"], "reps": args.reps, "call_ms_median": statistics.median(calls) * 1e3,
           "kernels_ms_median": statistics.median(kernels) * 1e3, "kernels_ms_min": min(kernels) * 1e3, "kernels_ms_max": max(kernels) * 1e3,
           "alg_gb": alg / 1e9, "launches": stats["launches"]}
    results.append(row)
    print(f"{name:46s} {n / 1e6:5.0f} M rows -> {stats['rows_out']:>9d} groups: call {row['call_ms_median']:8.1f} ms, kernels "
          f"{row['kernels_ms_median']:8.1f} ms (min {row['kernels_ms_min']:.1f}, max {row['kernels_ms_max']:.1f}), {alg / 1e9:6.1f} alg GB, "
          f"{stats['launches']} launches", flush=True)
rec.release()

if args.json:
    with open(args.json, "w") as fh:
        json.dump(results, fh, indent=1)
