"""ORDER BY throughput: chq.sort_record on device-resident batches of the reference's sample
shape (id: Int32, value1: Utf8 of 8 letters, value2: Float32; create_sample_data.rs), against torch.sort(stable=True) +
index_select of the same columns on the same device (the rocPRIM-based yardstick), timed alternately in one process.

  sort by value2          100 M rows
  sort by id DESC, value1 100 M rows
  sort by value1          100 M rows
  sort by a Float32 key     1 B rows (key + Int32 row id)

Times are steady state (one warm-up call per shape): `call` is the host clock around the call, which ends in a stream
synchronisation; `kernels` is the library's own event pair around its launches (context option time_kernels).  `alg GB`
is the bytes the library's pass structure reads and writes (chq_call_stats); `of peak` = those bytes at 8 TB/s over the
kernel time.  torch's time covers the sort and the column gathers only; its keys are prepared outside the timing.
usage: python bench/micro/sort.py [--rows N] [--big-rows N] [--reps R] [--json PATH]"""
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
ap.add_argument("--big-rows", type=int, default=1_000_000_000)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--json", default=None)
args = ap.parse_args()

import torch   # noqa: E402

dev = torch.device("cuda", 0)
ctx = chq.Context(0)
ctx.set_option("time_kernels", 1)
results = []


def sample(n, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    ids = torch.arange(n, dtype=torch.int32, device=dev)
    letters = torch.randint(ord("a"), ord("z") + 1, (n, 8), dtype=torch.uint8, device=dev, generator=g)
    offs = torch.arange(n + 1, dtype=torch.int32, device=dev) * 8
    v2 = torch.rand(n, device=dev, generator=g) * 100
    torch.cuda.synchronize()
    rec = chq.DeviceRecordBatch.from_device_pointers(
        [("id", "i", ids.data_ptr()), ("value1", "u", offs.data_ptr(), letters.data_ptr()), ("value2", "f", v2.data_ptr())], n, ctx=ctx,
        keepalive=[ids, letters, offs, v2])
    return rec, ids, letters, v2


def be_key(letters):
    """the 8 letters as one int64 whose signed order is their byte order (torch has no unsigned 64-bit sort)"""
    x = letters.to(torch.int64)
    k = torch.zeros(letters.shape[0], dtype=torch.int64, device=dev)
    for b in range(8):
        k = (k << 8) | x[:, b]
    return k ^ (-(1 << 63))


def time_chq(rec, order_by):
    best, kernels, stats = 1e9, 1e9, None
    out = chq.sort_record(rec, [[]] * rec.num_columns, order_by, ctx=ctx)   # warm-up
    out.release()
    for _ in range(args.reps):
        t0 = time.perf_counter()
        out = chq.sort_record(rec, [[]] * rec.num_columns, order_by, ctx=ctx)
        dt = time.perf_counter() - t0
        stats = ctx.last_stats()
        out.release()
        best = min(best, dt)
        kernels = min(kernels, stats["kernel_ns"] * 1e-9)
    return best, kernels, stats


def time_torch(fn):
    fn()
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


def report(name, n, chq_t, torch_t):
    call, kern, st = chq_t
    alg = st["bytes_read_alg"] + st["bytes_written_alg"]
    row = {"case": name, "rows": n, "chq_call_ms": call * 1e3, "chq_kernels_ms": kern * 1e3, "chq_rows_per_s": n / call,
           "alg_gb": alg / 1e9, "of_peak": alg / PEAK / kern if kern > 0 else None, "launches": st["launches"],
           "torch_ms": torch_t * 1e3, "chq_kernels_over_torch": kern / torch_t}
    results.append(row)
    print(f"{name:28s} {n / 1e6:7.0f} M rows: chq call {call * 1e3:8.1f} ms ({n / call / 1e9:.2f} G rows/s), kernels "
          f"{kern * 1e3:8.1f} ms, {alg / 1e9:6.1f} alg GB = {100 * alg / PEAK / kern:4.1f} % of 8 TB/s, {st['launches']} launches | "
          f"torch sort + gather {torch_t * 1e3:8.1f} ms | chq / torch {kern / torch_t:.2f}", flush=True)


def key(name, asc=True):
    return A.OrderByExpr(A.ident(name), asc, None)


n = args.rows
rec, ids, letters, v2 = sample(n)
v1_key = be_key(letters)
v1_words = letters.view(torch.int64).view(-1)
torch.cuda.synchronize()


def gather_all(idx):
    return ids.index_select(0, idx), v1_words.index_select(0, idx), v2.index_select(0, idx)


cases = [
    ("value2", [key("value2")], lambda: gather_all(torch.sort(v2, stable=True)[1])),
    ("id DESC, value1", [key("id", False), key("value1")],
     lambda: gather_all((lambda p: p.index_select(0, torch.sort(-ids.index_select(0, p).to(torch.int64), stable=True)[1]))(
         torch.sort(v1_key, stable=True)[1]))),
    ("value1", [key("value1")], lambda: gather_all(torch.sort(v1_key, stable=True)[1])),
]
for name, order_by, tfn in cases:
    c = time_chq(rec, order_by)      # alternate: ours, then torch's, shape by shape
    t = time_torch(tfn)
    report(name, n, c, t)
rec.release()
del rec, ids, letters, v2, v1_key, v1_words
torch.cuda.empty_cache()

if args.big_rows > 0:
    nb = args.big_rows
    g = torch.Generator(device=dev).manual_seed(1)
    f = torch.rand(nb, device=dev, generator=g) * 100
    rows = torch.arange(nb, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    big = chq.DeviceRecordBatch.from_device_pointers([("k", "f", f.data_ptr()), ("row", "i", rows.data_ptr())], nb, ctx=ctx,
                                                     keepalive=[f, rows])
    c = time_chq(big, [key("k")])
    t = time_torch(lambda: (lambda p: (f.index_select(0, p), rows.index_select(0, p)))(torch.sort(f, stable=True)[1]))
    report("Float32 key", nb, c, t)
    big.release()

if args.json:
    with open(args.json, "w") as fh:
        json.dump(results, fh, indent=1)
