"""LEFT / FULL / SEMI / ANTI JOIN next to INNER on the same inputs: chq.join_records(how=...) on
device-resident batches of the reference's sample shape, the three inputs of bench/micro/join.py with rows taken out so
that the new kinds have something to pad.

  fact x half dimension on bucket   100 M rows (the sample columns plus bucket = id % 1000) x a dimension table that holds
                                    only 500 of the 1 000 buckets: INNER, LEFT, SEMI, ANTI
  1 : 1 on a unique Int32 id        10 M x 10 M rows less 10 % of the ids on each side (two independent draws), the right
                                    side shuffled: INNER, LEFT, FULL

Times are steady state (one warm-up call per case and kind): `call` is the host clock around the call, `kernels` the
library's own event pair around its launches (context option time_kernels); `alg GB` is the bytes the library's pass
structure reads and writes (chq_call_stats).  Every repetition is reported, not only the best.
usage: python bench/micro/outer_join.py [--fact-rows N] [--rows N] [--reps R] [--json PATH]"""
import argparse
import json
import sys
import time

sys.path.insert(0, ".")
import chapterhouseqe_amd as chq   # noqa: E402
from chapterhouseqe_amd import sqlast as A   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--fact-rows", type=int, default=100_000_000)
ap.add_argument("--rows", type=int, default=10_000_000)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--json", default=None)
args = ap.parse_args()

import torch   # noqa: E402

dev = torch.device("cuda", 0)
ctx = chq.Context(0)
ctx.set_option("time_kernels", 1)
results = []
g = torch.Generator(device=dev).manual_seed(0)


def sample(n):
    """the reference's sample columns for n rows, as torch tensors"""
    ids = torch.arange(n, dtype=torch.int32, device=dev)
    letters = torch.randint(ord("a"), ord("z") + 1, (n, 8), dtype=torch.uint8, device=dev, generator=g)
    v2 = torch.rand(n, device=dev, generator=g) * 100
    return ids, letters, v2


def wrap(cols, n):
    """(name, format, tensor[, bytes tensor]) -> a device batch over the tensors' memory"""
    keep = [t for c in cols for t in c[2:]]
    return chq.DeviceRecordBatch.from_device_pointers([(c[0], c[1]) + tuple(t.data_ptr() for t in c[2:]) for c in cols], n, ctx=ctx, keepalive=keep)


def offsets(n):
    return torch.arange(n + 1, dtype=torch.int32, device=dev) * 8


def run(case, left, right, key, how):
    la, ra = [[]] * left.num_columns, [[]] * right.num_columns
    keys = [(A.ident(key), A.ident(key))]
    chq.join_records(left, la, right, ra, keys, ctx=ctx, how=how).release()   # warm-up
    calls, kernels, stats = [], [], None
    for _ in range(args.reps):
        t0 = time.perf_counter()
        out = chq.join_records(left, la, right, ra, keys, ctx=ctx, how=how)
        calls.append((time.perf_counter() - t0) * 1e3)
        stats = ctx.last_stats()
        out.release()
        kernels.append(stats["kernel_ns"] * 1e-6)
    alg = stats["bytes_read_alg"] + stats["bytes_written_alg"]
    results.append({"case": case, "how": how, "left_rows": left.num_rows, "right_rows": right.num_rows, "rows_out": stats["rows_out"],
                    "chq_call_ms": calls, "chq_kernels_ms": kernels, "alg_gb": alg / 1e9, "launches": stats["launches"]})
    print(f"{case:34s} {how:6s} {left.num_rows:>10d} x {right.num_rows:>9d} rows -> {stats['rows_out']:>10d} rows: kernels min {min(kernels):7.2f} "
          f"median {sorted(kernels)[len(kernels) // 2]:7.2f} max {max(kernels):7.2f} ms, call min {min(calls):7.2f} ms, {alg / 1e9:6.1f} alg GB, "
          f"{stats['launches']} launches", flush=True)


# ---- (a) fact x a dimension table that covers half the buckets
n = args.fact_rows
ids, letters, v2 = sample(n)
bucket = ids % 1000
offs = offsets(n)
dim_bucket = torch.randperm(1000, device=dev, generator=g).to(torch.int32)[:500].contiguous()
dim_weight = torch.rand(500, device=dev, generator=g)
torch.cuda.synchronize()
fact = wrap([("id", "i", ids), ("value1", "u", offs, letters), ("value2", "f", v2), ("bucket", "i", bucket)], n)
dim = wrap([("bucket", "i", dim_bucket), ("weight", "f", dim_weight)], 500)
for how in ("inner", "left", "semi", "anti"):
    run("fact x half dimension on bucket", fact, dim, "bucket", how)
fact.release()
dim.release()
del ids, letters, v2, bucket, offs, fact, dim
torch.cuda.empty_cache()

# ---- (b) 1 : 1 on the id, 10 % of the ids removed on each side, the right side shuffled
n = args.rows
ids, letters, v2 = sample(n)
keep_l = torch.nonzero(torch.rand(n, device=dev, generator=g) >= 0.1).squeeze(1)
keep_r = torch.nonzero(torch.rand(n, device=dev, generator=g) >= 0.1).squeeze(1)
keep_r = keep_r[torch.randperm(keep_r.shape[0], device=dev, generator=g)]
nl, nr = keep_l.shape[0], keep_r.shape[0]
l_ids, l_letters, l_v2 = ids.index_select(0, keep_l), letters.index_select(0, keep_l).contiguous(), v2.index_select(0, keep_l)
r_ids, r_letters, r_v2 = ids.index_select(0, keep_r), letters.index_select(0, keep_r).contiguous(), torch.rand(nr, device=dev, generator=g)
l_offs, r_offs = offsets(nl), offsets(nr)
torch.cuda.synchronize()
left = wrap([("id", "i", l_ids), ("value1", "u", l_offs, l_letters), ("value2", "f", l_v2)], nl)
right = wrap([("id", "i", r_ids), ("value1", "u", r_offs, r_letters), ("value2", "f", r_v2)], nr)
for how in ("inner", "left", "full"):
    run("1 : 1 on Int32 id, 10 % removed", left, right, "id", how)
left.release()
right.release()

if args.json:
    with open(args.json, "w") as fh:
        json.dump(results, fh, indent=1)
