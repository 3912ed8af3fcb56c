"""DATE / TIMESTAMP literals, EXTRACT and date_trunc on a device-resident batch in HBM: `ts`
Timestamp(us) spread evenly over the 20 years 2005 - 2024 and `d` Date32, the day of `ts`; 100 M rows by default.  The batch is
generated here; nothing is read from disk.

Timed, with the host clock around the call (the temporal kernel, the read-back of its null count, the kernels of the rest of the
expression and the export of the result), medians of --reps repetitions after a warm-up:

  select extract(year from ts)              Int64 in, Int32 out: 8 bytes read, 4 written per row
  select date_trunc('month', ts)            Int64 in, Int64 out: 8 read, 8 written
  where extract(dow from ts) = 0            the field into a temporary column, then the ordinary filter over both columns
  where ts >= TIMESTAMP a and ts < TIMESTAMP b   about 10 % of the rows: no temporal kernel, an Int64 compare in the filter program

Each beside lines measured in the same process on the same buffers:

  copy     torch.clone of a column of the output's size
  cast     select cast(d32 as bigint) -- bench/micro/cast.py's line, the nearest typed operation of the same launch structure
  twin     the literal filter's twin: the same buffers typed Int64 / Int32, the bounds written as integers

A second pass with the context option `time_kernels` reads the library's own event pair around its launches (kernel_ms) and the
algorithmic bytes of the call (chq_call_stats), from which GB/s against the copy line follow.

usage: python bench/micro/temporal.py [--rows N] [--reps R] [--json PATH]"""
import argparse
import datetime
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
EPOCH = datetime.datetime(1970, 1, 1)


def micros(y, m, d):
    return (datetime.datetime(y, m, d) - EPOCH) // datetime.timedelta(microseconds=1)


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


def report(label, t, copy=None, extra=None):
    med, lo, hi = t
    r = {"rows": n, "what": label, "ms": med * 1e3, "min_ms": lo * 1e3, "max_ms": hi * 1e3}
    if copy is not None:
        r["fraction_of_copy"] = copy["ms"] / r["ms"]
    r.update(extra or {})
    results.append(r)
    tail = f"  {r['fraction_of_copy']:.3f} of copy" if copy else ""
    if extra:
        tail += f"  kernels {extra['kernel_ms']:.3f} ms, {extra['launches']} launches, {extra['alg_gb']:.2f} GB -> {extra['kernel_gb_s']:.0f} GB/s"
    print(f"  {label:64s} {r['ms']:9.3f} ms  ({r['min_ms']:.3f} .. {r['max_ms']:.3f}){tail}", flush=True)
    return r


lo_us, hi_us = micros(2005, 1, 1), micros(2025, 1, 1)
g = torch.Generator(device=dev).manual_seed(15)
ts = torch.randint(lo_us, hi_us, (n,), dtype=torch.int64, device=dev, generator=g)
d = torch.div(ts, 86400 * 10**6, rounding_mode="floor").to(torch.int32)
torch.cuda.synchronize()
rec = chq.DeviceRecordBatch.from_device_buffers(
    [{"name": "ts", "format": "tsu:", "values": ts.data_ptr()}, {"name": "d", "format": "tdD", "values": d.data_ptr()}], n, ctx, keepalive=[ts, d])
twin = chq.DeviceRecordBatch.from_device_buffers(
    [{"name": "ts", "format": "l", "values": ts.data_ptr()}, {"name": "d", "format": "i", "values": d.data_ptr()}], n, ctx, keepalive=[ts, d])
aliases = [[]] * 2
print(f"{n} rows", flush=True)


def project(sql, batch=rec):
    fields = parse_select(f"select {sql} from t").projection

    def run():
        out = chq.project_record(fields, batch, aliases, ctx=ctx)
        out.release()
    return run


def where(sql, batch=rec):
    pred = parse_select(f"select * from t where {sql}").selection

    def run():
        out = chq.filter_record(batch, aliases, pred, ctx=ctx)
        out.release()
    return run


def kernels(fn):
    """the library's own event pair and byte counters over --reps more calls"""
    ctx.set_option("time_kernels", 1)
    fn()
    ns, st = [], None
    for _ in range(args.reps):
        fn()
        st = ctx.last_stats()
        ns.append(st["kernel_ns"])
    ctx.set_option("time_kernels", 0)
    k = statistics.median(ns)
    gb = (st["bytes_read_alg"] + st["bytes_written_alg"]) / 1e9
    return {"kernel_ms": k / 1e6, "launches": st["launches"], "alg_gb": gb, "kernel_gb_s": gb / (k / 1e9) if k else 0.0}


def line(label, fn, copy):
    t = timed(fn)
    return report(label, t, copy, kernels(fn))


big = torch.zeros(n, dtype=torch.int64, device=dev)
copy8 = report("copy (torch.clone of one 8-byte column)", timed(sync(lambda: big.clone())))
del big
copy4 = report("copy (torch.clone of one 4-byte column)", timed(sync(lambda: d.clone())))
line("select cast(d as bigint)   (on the Int32 twin; cast.py's line)", project("cast(d as bigint)", twin), copy8)
line("select extract(year from ts)", project("extract(year from ts)"), copy4)
line("select extract(year from d)", project("extract(year from d)"), copy4)
line("select date_trunc('month', ts)", project("date_trunc('month', ts)"), copy8)
line("select date_trunc('month', d)", project("date_trunc('month', d)"), copy4)
line("where d = 0   (the filter alone on the twin, nothing kept)", where("d = 0", twin), copy8)
line("where extract(dow from ts) = 0", where("extract(dow from ts) = 0"), copy8)
a, b = micros(2010, 1, 1), micros(2012, 1, 1)
lit_fn = where("ts >= TIMESTAMP '2010-01-01 00:00:00' and ts < TIMESTAMP '2012-01-01 00:00:00'")
twin_fn = where(f"ts >= {a} and ts < {b}", twin)


def alternating(f1, f2):
    """the two calls in turn, rep by rep, so that neither has the quieter half of the window"""
    f1(); f2()   # warm-up
    t1, t2 = [], []
    for _ in range(args.reps):
        for f, ts_ in ((f1, t1), (f2, t2)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            ts_.append(time.perf_counter() - t0)
    return (statistics.median(t1), min(t1), max(t1)), (statistics.median(t2), min(t2), max(t2))


t_lit, t_twin = alternating(lit_fn, twin_fn)
lit = report("where ts >= TIMESTAMP '2010-01-01 00:00:00' and ts < TIMESTAMP '2012-01-01 00:00:00'", t_lit, copy8, kernels(lit_fn))
tw = report(f"where ts >= {a} and ts < {b}   (the Int64 twin, calls alternating)", t_twin, copy8, kernels(twin_fn))
inside = tw["min_ms"] <= lit["ms"] <= tw["max_ms"]
print(f"  literal filter {lit['ms']:.3f} ms against its twin's {tw['min_ms']:.3f} .. {tw['max_ms']:.3f} ms: {'inside' if inside else 'OUTSIDE'}", flush=True)
results.append({"what": "literal filter inside its twin's min..max", "value": inside})
rec.release()
twin.release()
if args.json:
    with open(args.json, "w") as f:
        json.dump(results, f, indent=1)
ctx.close()
