"""CAST / TRY_CAST on a device-resident batch of the reference's sample shape (id: Int32, value1:
Utf8, value2: Float32), 100 M rows by default, in HBM.  value1 holds digit strings here (1 to 3 digits, the decimal of
id % 200), so that `where cast(value1 as int) > 5` parses every row.

Timed, with the host clock around the call (the cast kernel, count_bits_kernel over its validity, the read-back of the counts,
the kernels of the rest of the expression and the export of the result):

  select cast(id as bigint)                 Int32 -> Int64: 4 bytes read, 8 written per row
  select cast(value2 as int)                Float32 -> Int32 with its NaN / range check: 4 read, 4 written
  where cast(value1 as int) > 5             Utf8 -> Int32 into a temporary column, then the ordinary filter over all columns
  select cast(id as varchar)                Int32 -> Utf8: lengths, the offsets scan, the bytes

Each beside two lines measured in the same run on the same batch:

  copy     torch.clone of a column of the output's size (the Utf8 output: offsets + data)
  torch    `.to(dtype)` where torch has the conversion (Int32 -> Int64, Float32 -> Int32)

usage: python bench/micro/cast.py [--rows N] [--reps R] [--json PATH]"""
import argparse
import json
import statistics
import sys
import time

sys.path.insert(0, ".")
import chapterhouseqe_amd as chq   # noqa: E402
from chapterhouseqe_amd.sqlparse import parse_select   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=100_000_000)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--json", default=None)
args = ap.parse_args()

import torch   # noqa: E402

dev = torch.device("cuda", 0)
ctx = chq.Context(0)
results = []
n = args.rows


def timed(fn):
    fn()   # warm-up
    ts = []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts), max(ts)


def sync(fn):
    def run():
        r = fn()
        torch.cuda.synchronize()
        del r
    return run


def report(label, t, copy=None):
    med, lo, hi = t
    r = {"rows": n, "what": label, "ms": med * 1e3, "min_ms": lo * 1e3, "max_ms": hi * 1e3}
    if copy is not None:
        r["fraction_of_copy"] = copy["ms"] / r["ms"]
    results.append(r)
    print(f"  {label:64s} {r['ms']:9.3f} ms  ({r['min_ms']:.3f} .. {r['max_ms']:.3f})" + (f"  {r['fraction_of_copy']:.3f} of copy" if copy else ""), flush=True)
    return r


g = torch.Generator(device=dev).manual_seed(14)
ids = torch.arange(n, dtype=torch.int32, device=dev)
v2 = torch.rand(n, device=dev, generator=g) * 200 - 100
# value1: the decimal of id % 200, 1 to 3 digits, no padding
code = ids % 200
lens = 1 + (code >= 10).to(torch.int32) + (code >= 100).to(torch.int32)
offs = torch.zeros(n + 1, dtype=torch.int32, device=dev)
torch.cumsum(lens, 0, out=offs[1:])
total = int(offs[-1].item())
digits = torch.empty(total, dtype=torch.uint8, device=dev)
start = offs[:-1].to(torch.int64)
last = start + (lens - 1)
digits[last] = (48 + code % 10).to(torch.uint8)
two = code >= 10
digits[(last - 1)[two]] = (48 + (code // 10) % 10).to(torch.uint8)[two]
three = code >= 100
digits[start[three]] = (48 + code // 100).to(torch.uint8)[three]
del start, last, two, three, lens, code
torch.cuda.synchronize()
rec = chq.DeviceRecordBatch.from_device_buffers(
    [{"name": "id", "format": "i", "values": ids.data_ptr()}, {"name": "value1", "format": "u", "values": offs.data_ptr(), "data": digits.data_ptr()},
     {"name": "value2", "format": "f", "values": v2.data_ptr()}], n, ctx, keepalive=[ids, digits, offs, v2])
aliases = [[]] * 3
print(f"{n} rows, value1 of {total} bytes", flush=True)


def project(sql):
    fields = parse_select(f"select {sql} from t").projection

    def run():
        out = chq.project_record(fields, rec, aliases, ctx=ctx)
        out.release()
    return run


def where(sql):
    pred = parse_select(f"select * from t where {sql}").selection

    def run():
        out = chq.filter_record(rec, aliases, pred, ctx=ctx)
        out.release()
    return run


big = torch.zeros(n, dtype=torch.int64, device=dev)
copy8 = report("copy (torch.clone of one 8-byte column)", timed(sync(lambda: big.clone())))
report("torch: id.to(int64)", timed(sync(lambda: ids.to(torch.int64))), copy8)
report("select cast(id as bigint)", timed(project("cast(id as bigint)")), copy8)
copy4 = report("copy (torch.clone of one 4-byte column)", timed(sync(lambda: v2.clone())))
report("torch: value2.to(int32)", timed(sync(lambda: v2.to(torch.int32))), copy4)
del big
report("select cast(value2 as int)", timed(project("cast(value2 as int)")), copy4)
report("where value2 > 5.0   (the filter alone, no cast)", timed(where("value2 > 5.0")), copy4)
report("where cast(value1 as int) > 5", timed(where("cast(value1 as int) > 5")), copy4)


# Int32 -> Utf8: the copy line is of the output's own size -- the digits of 0 .. n - 1 (k + 1 digits from 10^k up) and the offsets
out_bytes = 1 + sum((k + 1) * (min(n, 10 ** (k + 1)) - min(n, 10 ** k)) for k in range(10))
buf = torch.empty(out_bytes, dtype=torch.uint8, device=dev)


def clone_out():
    x, y = offs.clone(), buf.clone()
    torch.cuda.synchronize()
    del x, y


copys = report(f"copy (torch.clone of the Utf8 output: offsets + {out_bytes} bytes)", timed(clone_out))
report("select cast(id as varchar)", timed(project("cast(id as varchar)")), copys)
rec.release()
if args.json:
    with open(args.json, "w") as f:
        json.dump(results, f, indent=1)
ctx.close()
