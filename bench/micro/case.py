"""CASE / COALESCE on a device-resident batch of the reference's sample shape (id: Int32, value1:
Utf8 of random lower-case letters, value2: Float32, 6 % of value2 null), 100 M rows by default, in HBM.

Timed, with the host clock around project_record (the conditions' temporaries, the mask and select kernels, their read-backs
and the export of the result):

  select case when value2 > 10.0 then value2 else 0.0 end         one Float32 select under one condition
  select case when id < A then 1 when id < B then 2 when id < C then 3 else 4 end      a three-WHEN Int32 bucket on id
  select coalesce(value2, 0.0)                                      fills the nulls
  select case when id % 2 = 0 then value1 else 'odd' end            a Utf8 result: rows, scan, gather (8- and 100-byte strings)
  select case when id % 7 <> 0 then id / (id % 7) else 0 end        guarded: the division runs under the take mask
  select case when id % 7 <> 0 then value2 / 7.0 else 0.0 end       the same shape without a guard need: float arithmetic cannot
                                                                    fail (any integer division is checked, so it is guarded)

Two lines to measure against, in the same run on the same batch:

  copy          torch.clone of an output-sized column (4 bytes a row; the Utf8 shape: offsets + data of value1)
  torch.where   torch.where on PRECOMPUTED masks: what the select kernel alone would cost at best

usage: python bench/micro/case.py [--rows N] [--wide-rows N] [--reps R] [--json PATH]"""
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
ap.add_argument("--wide-rows", type=int, default=20_000_000, help="rows of the 100-byte string shape")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--json", default=None)
args = ap.parse_args()

import torch   # noqa: E402

dev = torch.device("cuda", 0)
ctx = chq.Context(0)
results = []


def timed(fn):
    fn()   # warm-up
    ts = []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts), max(ts)


def run_shape(name, n, width, with_numeric):
    if n <= 0:
        return
    g = torch.Generator(device=dev).manual_seed(width)
    ids = torch.arange(n, dtype=torch.int32, device=dev)
    letters = torch.randint(ord("a"), ord("z") + 1, (n * width,), dtype=torch.uint8, device=dev, generator=g)
    offs = torch.arange(n + 1, dtype=torch.int64, device=dev).mul_(width).to(torch.int32)
    v2 = torch.rand(n, device=dev, generator=g) * 100
    # validity of value2: 6 % nulls, packed little-endian
    valid = torch.rand(n + (-n) % 8, device=dev, generator=g) >= 0.06
    packed = (valid.view(-1, 8).to(torch.uint8) << torch.arange(8, device=dev, dtype=torch.uint8)).sum(1, dtype=torch.uint8)
    nulls = int(n - valid[:n].sum().item())
    torch.cuda.synchronize()
    rec = chq.DeviceRecordBatch.from_device_buffers(
        [{"name": "id", "format": "i", "values": ids.data_ptr()}, {"name": "value1", "format": "u", "values": offs.data_ptr(), "data": letters.data_ptr()},
         {"name": "value2", "format": "f", "values": v2.data_ptr(), "validity": packed.data_ptr(), "null_count": nulls, "nullable": True}], n, ctx,
        keepalive=[ids, letters, offs, v2, packed])
    aliases = [[]] * 3
    print(f"{name}: {n} rows, value1 of {width} bytes, {nulls} nulls in value2", flush=True)

    def report(label, t, copy=None):
        med, lo, hi = t
        r = {"shape": name, "rows": n, "width": width, "what": label, "ms": med * 1e3, "min_ms": lo * 1e3, "max_ms": hi * 1e3}
        if copy is not None:
            r["fraction_of_copy"] = copy["ms"] / r["ms"]
        results.append(r)
        print(f"  {label:72s} {r['ms']:9.3f} ms  ({r['min_ms']:.3f} .. {r['max_ms']:.3f})" + (f"  {r['fraction_of_copy']:.3f} of copy" if copy else ""), flush=True)
        return r

    def project(sql):
        fields = parse_select(f"select {sql} from t").projection

        def run():
            out = chq.project_record(fields, rec, aliases, ctx=ctx)
            out.release()
        return run

    def sync(fn):
        def run():
            r = fn()
            torch.cuda.synchronize()
            del r
        return run

    if with_numeric:
        copy4 = report("copy (torch.clone of one 4-byte column)", timed(sync(lambda: v2.clone())))
        m1 = v2 > 10.0
        a, b, c = n // 4, n // 2, 3 * (n // 4)
        b1, b2, b3 = ids < a, (ids >= a) & (ids < b), (ids >= b) & (ids < c)
        zero = torch.zeros((), device=dev)
        one, two, three, four = (torch.full((), k, dtype=torch.int32, device=dev) for k in (1, 2, 3, 4))
        report("torch.where(mask, value2, 0.0), mask precomputed", timed(sync(lambda: torch.where(m1, v2, zero))), copy4)
        report("torch.where x 3, masks precomputed (the bucket)", timed(sync(lambda: torch.where(b1, one, torch.where(b2, two, torch.where(b3, three, four))))), copy4)
        del m1, b1, b2, b3
        report("select case when value2 > 10.0 then value2 else 0.0 end", timed(project("case when value2 > 10.0 then value2 else 0.0 end")), copy4)
        report("select three-WHEN Int32 bucket on id", timed(project(f"case when id < {a} then 1 when id < {b} then 2 when id < {c} then 3 else 4 end")), copy4)
        report("select coalesce(value2, 0.0)", timed(project("coalesce(value2, 0.0)")), copy4)
        report("select case when id % 7 <> 0 then id / (id % 7) else 0 end   (guarded)", timed(project("case when id % 7 <> 0 then id / (id % 7) else 0 end")), copy4)
        report("select case when id % 7 <> 0 then value2 / 7.0 else 0.0 end  (no guard)", timed(project("case when id % 7 <> 0 then value2 / 7.0 else 0.0 end")), copy4)

    def clone_str():
        x, y = offs.clone(), letters.clone()
        torch.cuda.synchronize()
        del x, y
    copys = report(f"copy (torch.clone of value1: offsets + {width}-byte data)", timed(clone_str))
    report(f"select case when id % 2 = 0 then value1 else 'odd' end   ({width}-byte strings)", timed(project("case when id % 2 = 0 then value1 else 'odd' end")), copys)
    rec.release()


run_shape("short", args.rows, 8, True)
torch.cuda.empty_cache()
run_shape("wide", args.wide_rows, 100, False)
if args.json:
    with open(args.json, "w") as f:
        json.dump(results, f, indent=1)
ctx.close()
