"""INNER JOIN throughput: chq.join_records on device-resident batches of the reference's sample shape
(id: Int32, value1: Utf8 of 8 letters, value2: Float32; create_sample_data.rs), against torch on the same device -- stable
torch.sort of the right keys, two searchsorted of the left keys, repeat_interleave for the left row of every output,
index_select of every column of both sides -- timed alternately in one process.

  fact x dimension on bucket   100 M rows (the sample columns plus bucket = id % 1000) x a 1 000-row dimension table
  1 : 1 on a unique Int32 id    10 M x 10 M rows, the right side shuffled
  1 : 1 on the 8-byte value1    10 M x 10 M rows, the right side shuffled

Times are steady state (one warm-up call per case): `call` is the host clock around the call, which ends in a stream
synchronisation; `kernels` is the library's own event pair around its launches (context option time_kernels), the key
concatenation and the sort included.  `alg GB` is the bytes the library's pass structure reads and writes
(chq_call_stats); `of peak` = those bytes at 8 TB/s over the kernel time.  torch's keys are prepared outside the timing (the
8 letters as one int64), and its Utf8 column is an (n, 8) byte matrix: it rebuilds no offsets.
usage: python bench/micro/join.py [--fact-rows N] [--rows N] [--reps R] [--json PATH]"""
import argparse
import json
import sys
import time

sys.path.insert(0, ".")
import chapterhouseqe_amd as chq   # noqa: E402
from chapterhouseqe_amd import sqlast as A   # noqa: E402

PEAK = 8.0e12

ap = argparse.ArgumentParser()
ap.add_argument("--fact-rows", type=int, default=100_000_000)
ap.add_argument("--rows", type=int, default=10_000_000)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--json", default=None)
args = ap.parse_args()

import torch   # noqa: E402

dev = torch.device("cuda", 0)
ctx = chq.Context(0)
ctx.set_option("time_kernels", 1)
results = []
g = torch.Generator(device=dev).manual_seed(0)


def be_key(x8):
    """the 8 letters as one int64 whose signed order is their byte order (torch has no unsigned 64-bit sort)"""
    x = x8.to(torch.int64)
    k = torch.zeros(x8.shape[0], dtype=torch.int64, device=dev)
    for b in range(8):
        k = (k << 8) | x[:, b]
    return k ^ (-(1 << 63))


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


def time_chq(left, right, keys):
    la, ra = [[]] * left.num_columns, [[]] * right.num_columns
    best, kernels, stats = 1e9, 1e9, None
    chq.join_records(left, la, right, ra, keys, ctx=ctx).release()   # warm-up
    for _ in range(args.reps):
        t0 = time.perf_counter()
        out = chq.join_records(left, la, right, ra, keys, ctx=ctx)
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


def torch_join(lkey, rkey, lcols, rcols):
    """stable sort of the right keys; the run of every left key by two binary searches; the pairs left-major"""
    skey, rperm = torch.sort(rkey, stable=True)
    lo = torch.searchsorted(skey, lkey, right=False)
    cnt = torch.searchsorted(skey, lkey, right=True) - lo
    lidx = torch.repeat_interleave(torch.arange(lkey.shape[0], device=dev), cnt)
    off = torch.cumsum(cnt, 0) - cnt
    ridx = rperm.index_select(0, lo.index_select(0, lidx) + (torch.arange(lidx.shape[0], device=dev) - off.index_select(0, lidx)))
    return [c.index_select(0, lidx) for c in lcols] + [c.index_select(0, ridx) for c in rcols]


def report(name, nl, nr, chq_t, torch_t):
    call, kern, st = chq_t
    alg = st["bytes_read_alg"] + st["bytes_written_alg"]
    row = {"case": name, "left_rows": nl, "right_rows": nr, "rows_out": st["rows_out"], "chq_call_ms": call * 1e3, "chq_kernels_ms": kern * 1e3,
           "alg_gb": alg / 1e9, "of_peak": alg / PEAK / kern if kern > 0 else None, "launches": st["launches"],
           "torch_ms": torch_t * 1e3 if torch_t else None, "chq_kernels_over_torch": kern / torch_t if torch_t else None}
    results.append(row)
    torch_text = f"torch {torch_t * 1e3:8.1f} ms | chq / torch {kern / torch_t:.2f}" if torch_t else "torch: not measured"
    print(f"{name:30s} {nl / 1e6:5.0f} M x {nr:>9d} rows -> {st['rows_out']:>10d} rows: chq call {call * 1e3:8.1f} ms, kernels {kern * 1e3:8.1f} ms, "
          f"{alg / 1e9:6.1f} alg GB = {100 * alg / PEAK / kern:4.1f} % of 8 TB/s, {st['launches']} launches | {torch_text}", flush=True)


def offsets(n):
    return torch.arange(n + 1, dtype=torch.int32, device=dev) * 8


# ---- (a) fact x dimension on bucket
n = args.fact_rows
ids, letters, v2 = sample(n)
bucket = ids % 1000
offs = offsets(n)
dim_bucket = torch.randperm(1000, device=dev, generator=g).to(torch.int32)
dim_weight = torch.rand(1000, device=dev, generator=g)
torch.cuda.synchronize()
fact = wrap([("id", "i", ids), ("value1", "u", offs, letters), ("value2", "f", v2), ("bucket", "i", bucket)], n)
dim = wrap([("bucket", "i", dim_bucket), ("weight", "f", dim_weight)], 1000)
c = time_chq(fact, dim, [(A.ident("bucket"), A.ident("bucket"))])      # alternate: ours, then torch's, case by case
t = time_torch(lambda: torch_join(bucket, dim_bucket, [ids, letters, v2, bucket], [dim_bucket, dim_weight]))
report("fact x dimension on bucket", n, 1000, c, t)
fact.release()
dim.release()
del ids, letters, v2, bucket, offs, fact, dim
torch.cuda.empty_cache()

# ---- (b), (c) 1 : 1, the right side a shuffle of the left
n = args.rows
ids, letters, v2 = sample(n)
offs = offsets(n)
shuffle = torch.randperm(n, device=dev, generator=g)
r_ids, r_letters, r_v2 = ids.index_select(0, shuffle), letters.index_select(0, shuffle).contiguous(), torch.rand(n, device=dev, generator=g)
l_key, r_key = be_key(letters), be_key(r_letters)
torch.cuda.synchronize()
left = wrap([("id", "i", ids), ("value1", "u", offs, letters), ("value2", "f", v2)], n)
right = wrap([("id", "i", r_ids), ("value1", "u", offs, r_letters), ("value2", "f", r_v2)], n)
for name, col, lk, rk in (("1 : 1 on a unique Int32 id", "id", ids, r_ids), ("1 : 1 on the 8-byte value1", "value1", l_key, r_key)):
    c = time_chq(left, right, [(A.ident(col), A.ident(col))])
    t = time_torch(lambda: torch_join(lk, rk, [ids, letters, v2], [r_ids, r_letters, r_v2]))
    report(name, n, n, c, t)
left.release()
right.release()

if args.json:
    with open(args.json, "w") as fh:
        json.dump(results, fh, indent=1)
