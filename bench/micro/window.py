"""Window-function throughput: chq.window_record on a device-resident batch of the reference's
sample shape (id: Int32, value1: Utf8 of 8 letters, value2: Float32; create_sample_data.rs) plus `bucket` = id % 1000
materialised as an Int32 column, against a torch restatement on the same device -- stable torch.sort of the keys, segment
starts from unique_consecutive, cumsum or a shifted index, and a scatter back to input order -- timed alternately in one process.

  a  row_number() over (partition by bucket order by value2)                                  100 M rows, 1000 partitions
  b  sum(value2) over (partition by bucket order by id rows between unbounded preceding and current row)
  c  lag(value2, 1) over (order by id)                                                         one partition

Times are steady state (one warm-up call per query): `call` is the host clock around the call, which ends in a stream
synchronisation; `kernels` is the library's own event pair around its launches (context option time_kernels), the sort and
the pass-through copy of the four input columns included.  `alg GB` is the bytes the library's pass structure reads and
writes (chq_call_stats); `of peak` = those bytes at 8 TB/s over the kernel time.  torch's side returns the new column only:
it copies no input column, and its running sum is one Float64 cumsum over all rows minus the value in front of the partition.
usage: python bench/micro/window.py [--rows N] [--reps R] [--case a|b|c] [--no-torch] [--json PATH]"""
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
ap.add_argument("--case", default=None, help="run one query only (a, b or c): what a kernel trace is taken of")
ap.add_argument("--no-torch", action="store_true")
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


def time_chq(partition_by, order_by, items):
    best, kernels, stats = 1e9, 1e9, None
    chq.window_record(rec, ALIASES, partition_by, order_by, items, ctx=ctx).release()   # warm-up
    for _ in range(args.reps):
        t0 = time.perf_counter()
        out = chq.window_record(rec, ALIASES, partition_by, order_by, items, ctx=ctx)
        dt = time.perf_counter() - t0
        stats = ctx.last_stats()
        out.release()
        best = min(best, dt)
        kernels = min(kernels, stats["kernel_ns"] * 1e-9)
    return best, kernels, stats


def time_torch(fn):
    if args.no_torch:
        return None
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
    row = {"case": name, "rows": n, "chq_call_ms": call * 1e3, "chq_kernels_ms": kern * 1e3, "chq_rows_per_s": n / call,
           "alg_gb": alg / 1e9, "of_peak": alg / PEAK / kern if kern > 0 else None, "launches": st["launches"],
           "torch_ms": torch_t * 1e3 if torch_t else None, "chq_kernels_over_torch": kern / torch_t if torch_t else None}
    results.append(row)
    torch_text = f"torch {torch_t * 1e3:8.1f} ms | chq / torch {kern / torch_t:.2f}" if torch_t else "torch: not measured"
    print(f"{name:58s} {n / 1e6:5.0f} M rows: chq call {call * 1e3:8.1f} ms, kernels {kern * 1e3:8.1f} ms, "
          f"{alg / 1e9:6.1f} alg GB = {100 * alg / PEAK / kern:4.1f} % of 8 TB/s, {st['launches']} launches | {torch_text}", flush=True)


def segment_starts(skey):
    """the first sorted position of every position's run of equal keys"""
    pos = torch.arange(skey.shape[0], device=dev)
    counts = torch.unique_consecutive(skey, return_counts=True)[1]
    return pos, torch.repeat_interleave(torch.cumsum(counts, 0) - counts, counts)


def torch_row_number():
    p1 = torch.sort(v2, stable=True).indices                       # least significant key first
    skey, p2 = torch.sort(bucket.index_select(0, p1), stable=True)
    perm = p1.index_select(0, p2)
    pos, start = segment_starts(skey)
    out = torch.empty(n, dtype=torch.int64, device=dev)
    out[perm] = pos - start + 1
    return out


def torch_running_sum():
    skey, perm = torch.sort(bucket, stable=True)                   # (id is ascending already: the stable sort keeps it)
    pos, start = segment_starts(skey)
    x = v2.index_select(0, perm).to(torch.float64)
    cs = torch.cumsum(x, 0)
    before = cs.index_select(0, start) - x.index_select(0, start)  # the running total in front of the partition
    out = torch.empty(n, dtype=torch.float64, device=dev)
    out[perm] = cs - before
    return out


def torch_lag():
    perm = torch.sort(ids, stable=True).indices
    out = torch.full((n,), float("nan"), dtype=torch.float32, device=dev)   # (NaN stands for null)
    out[perm[1:]] = v2.index_select(0, perm[:-1])
    return out


K, F = A.WindowKind, A.WindowFrame
cases = [
    ("a", "row_number() over (partition by bucket order by value2)", [A.ident("bucket")], [A.OrderByExpr(A.ident("value2"))],
     [A.WindowItem(K.ROW_NUMBER, "rn")], torch_row_number),
    ("b", "sum(value2) over (partition by bucket order by id rows ..)", [A.ident("bucket")], [A.OrderByExpr(A.ident("id"))],
     [A.WindowItem(K.SUM, "running", A.ident("value2"), F.ROWS_TO_CURRENT)], torch_running_sum),
    ("c", "lag(value2, 1) over (order by id)", [], [A.OrderByExpr(A.ident("id"))],
     [A.WindowItem(K.LAG, "prev", A.ident("value2"), F.PARTITION, 1)], torch_lag),
]
for tag, name, partition_by, order_by, items, tfn in cases:
    if args.case and args.case != tag:
        continue
    c = time_chq(partition_by, order_by, items)      # alternate: ours, then torch's, query by query
    t = time_torch(tfn)
    report(f"{tag}  {name}", c, t)
rec.release()

if args.json:
    with open(args.json, "w") as fh:
        json.dump(results, fh, indent=1)
