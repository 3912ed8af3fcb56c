"""Hash partitioning throughput: chq.partition_records on a device-resident batch of the reference's
sample shape (id: Int32, value1: Utf8 of 8 letters, value2: Float32; create_sample_data.rs), against torch on the same device
-- a stable torch.sort of PRECOMPUTED partition ids and index_select of every column through its permutation -- timed
alternately in one process.  The torch path does not hash: its ids are uniform random bytes drawn outside the timing.

  by id into 8 partitions          by id into 256 partitions          by the 8-byte value1 into 8 partitions

Times are steady state (one warm-up call per case): `call` is the host clock around the call, which ends in a stream
synchronisation; `kernels` is the library's own event pair around its launches (context option time_kernels), the gathers of
every column included.  `alg GB` is the bytes the library's pass structure reads and writes (chq_call_stats); `of peak` =
those bytes at 8 TB/s over the kernel time.  torch's Utf8 column is an (n, 8) byte matrix: it rebuilds no offsets.
usage: python bench/micro/partition.py [--rows N] [--reps R] [--json PATH]"""
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
g = torch.Generator(device=dev).manual_seed(0)


def time_chq(rec, key, n_parts):
    al = [[]] * rec.num_columns
    best, kernels, stats = 1e9, 1e9, None
    for rep in range(args.reps + 1):   # (the first call is the warm-up)
        t0 = time.perf_counter()
        outs = chq.partition_records(rec, al, [A.ident(key)], n_parts, ctx=ctx)
        dt = time.perf_counter() - t0
        rows = [o.num_rows for o in outs]
        for o in outs:
            o.release()
        if rep == 0:
            continue
        stats = ctx.last_stats()
        best = min(best, dt)
        kernels = min(kernels, stats["kernel_ns"] * 1e-9)
    return best, kernels, stats, rows


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


def torch_partition(pids, cols):
    _, perm = torch.sort(pids, stable=True)
    return [c.index_select(0, perm) for c in cols]


n = args.rows
ids = torch.arange(n, dtype=torch.int32, device=dev)
letters = torch.randint(ord("a"), ord("z") + 1, (n, 8), dtype=torch.uint8, device=dev, generator=g)
v2 = torch.rand(n, device=dev, generator=g) * 100
offs = torch.arange(n + 1, dtype=torch.int32, device=dev) * 8
torch.cuda.synchronize()
cols = [("id", "i", ids), ("value1", "u", offs, letters), ("value2", "f", v2)]
keep = [t for c in cols for t in c[2:]]
rec = chq.DeviceRecordBatch.from_device_pointers([(c[0], c[1]) + tuple(t.data_ptr() for t in c[2:]) for c in cols], n, ctx=ctx, keepalive=keep)

for name, key, n_parts in (("by id into 8", "id", 8), ("by id into 256", "id", 256), ("by value1 (8 bytes) into 8", "value1", 8)):
    call, kern, st, rows = time_chq(rec, key, n_parts)      # alternate: ours, then torch's, case by case
    pids = torch.randint(0, n_parts, (n,), dtype=torch.uint8, device=dev, generator=g)
    t = time_torch(lambda: torch_partition(pids, [ids, letters, v2]))
    del pids
    alg = st["bytes_read_alg"] + st["bytes_written_alg"]
    results.append({"case": name, "rows": n, "partitions": n_parts, "min_rows": min(rows), "max_rows": max(rows), "chq_call_ms": call * 1e3,
                    "chq_kernels_ms": kern * 1e3, "alg_gb": alg / 1e9, "of_peak": alg / PEAK / kern if kern > 0 else None,
                    "launches": st["launches"], "torch_ms": t * 1e3 if t else None, "chq_kernels_over_torch": kern / t if t else None})
    torch_text = f"torch sort + index_select {t * 1e3:8.1f} ms | chq / torch {kern / t:.2f}" if t else "torch: not measured"
    print(f"{name:28s} {n / 1e6:5.0f} M rows -> {n_parts:3d} parts of {min(rows)}..{max(rows)} rows: chq call {call * 1e3:8.1f} ms, "
          f"kernels {kern * 1e3:8.1f} ms, {alg / 1e9:6.1f} alg GB = {100 * alg / PEAK / kern:4.1f} % of 8 TB/s, {st['launches']} launches | {torch_text}",
          flush=True)
rec.release()

if args.json:
    with open(args.json, "w") as fh:
        json.dump(results, fh, indent=1)
