"""LIKE throughput: `value1 like P` as a chq.filter_record predicate on a device-resident batch of
the reference's sample shape (id: Int32, value1: Utf8 of random lower-case letters, value2: Float32), in two shapes:

  wide    20 M rows x 100-byte value1 (the BASELINE wide-string config): like.hip's wave-per-row mode for patterns with a
          piece to search for, its lane-per-row mode for patterns that only look at the ends
  short   100 M rows x 8-byte value1: lane per row throughout

for the patterns 'ab%', '%ab', '%abc%' and '%a_c%x%'.  Per pattern: `filter ms` = the host clock around filter_record (the
LIKE kernel, the filter kernel that reads its Boolean column, and the copy of the surviving rows), `mask ms` = compute_value
of the predicate alone (the LIKE kernel, the pass that stores its column and the download of that bitmap), and the bytes of
(offsets + string data) per second for both.  Two lines to measure against, in the same run on the same batch:

  value1 >= 'n'                 the existing Utf8 comparison inside the filter's device program (keeps about half the rows,
                                so it copies far more than any of the patterns)
  pyarrow.compute.match_like    on the host, over the first --host-rows rows of the same column

usage: python bench/micro/like.py [--wide-rows N] [--short-rows N] [--host-rows N] [--reps R] [--json PATH]"""
import argparse
import json
import sys
import time

sys.path.insert(0, ".")
import chapterhouseqe_amd as chq   # noqa: E402
from chapterhouseqe_amd.sqlparse import parse_expr   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--wide-rows", type=int, default=20_000_000)
ap.add_argument("--short-rows", type=int, default=100_000_000)
ap.add_argument("--host-rows", type=int, default=2_000_000)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--json", default=None)
args = ap.parse_args()

import pyarrow as pa   # noqa: E402
import pyarrow.compute as pc   # noqa: E402
import torch   # noqa: E402

dev = torch.device("cuda", 0)
ctx = chq.Context(0)
PATTERNS = ["ab%", "%ab", "%abc%", "%a_c%x%"]
ALIASES = [[]] * 3
results = []


def best_of(fn):
    fn()   # warm-up
    best = 1e9
    for _ in range(args.reps):
        t0 = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t0)
    return best


def run_shape(name, n, width):
    if n <= 0:
        return
    g = torch.Generator(device=dev).manual_seed(width)
    ids = torch.arange(n, dtype=torch.int32, device=dev)
    letters = torch.randint(ord("a"), ord("z") + 1, (n * width,), dtype=torch.uint8, device=dev, generator=g)
    offs = torch.arange(n + 1, dtype=torch.int64, device=dev).mul_(width).to(torch.int32)
    v2 = torch.rand(n, device=dev, generator=g) * 100
    torch.cuda.synchronize()
    rec = chq.DeviceRecordBatch.from_device_pointers(
        [("id", "i", ids.data_ptr()), ("value1", "u", offs.data_ptr(), letters.data_ptr()), ("value2", "f", v2.data_ptr())], n, ctx=ctx,
        keepalive=[ids, letters, offs, v2])
    nbytes = 4 * (n + 1) + n * width
    print(f"{name}: {n} rows x {width}-byte value1, {nbytes / 1e9:.2f} GB of offsets + string data", flush=True)

    def filt(e):
        out = chq.filter_record(rec, ALIASES, e, ctx=ctx)
        rows = out.num_rows
        out.release()
        return rows

    def line(label, sql, mask=True):
        e = parse_expr(sql)
        kept = filt(e)
        t_filter = best_of(lambda: filt(e))
        t_mask = best_of(lambda: chq.compute_value(rec, ALIASES, e, ctx=ctx)) if mask else None
        r = {"shape": name, "rows": n, "width": width, "predicate": label, "rows_out": kept, "filter_ms": t_filter * 1e3,
             "filter_GBps": nbytes / t_filter / 1e9, "mask_ms": t_mask * 1e3 if mask else None, "mask_GBps": nbytes / t_mask / 1e9 if mask else None}
        results.append(r)
        print(f"  {label:28s} kept {kept:>11d}   filter {r['filter_ms']:9.3f} ms {r['filter_GBps']:8.1f} GB/s" +
              (f"   mask {r['mask_ms']:9.3f} ms {r['mask_GBps']:8.1f} GB/s" if mask else ""), flush=True)

    for p in PATTERNS:
        line(f"value1 like '{p}'", f"value1 like '{p}'")
    line("value1 >= 'n' (comparison)", "value1 >= 'n'")
    # the host line: the first host_rows rows of the same column
    m = min(n, args.host_rows)
    harr = pa.Array.from_buffers(pa.utf8(), m, [None, pa.py_buffer(offs[: m + 1].cpu().numpy().tobytes()), pa.py_buffer(letters[: m * width].cpu().numpy().tobytes())])
    hbytes = 4 * (m + 1) + m * width
    for p in PATTERNS:
        t0 = time.perf_counter()
        hits = pc.sum(pc.match_like(harr, p)).as_py()
        dt = time.perf_counter() - t0
        results.append({"shape": name, "rows": m, "width": width, "predicate": f"host match_like '{p}'", "rows_out": hits, "filter_ms": dt * 1e3,
                        "filter_GBps": hbytes / dt / 1e9})
        print(f"  host match_like '{p}' on {m} rows: {hits} hits, {dt * 1e3:9.3f} ms {hbytes / dt / 1e9:8.2f} GB/s", flush=True)
    rec.release()


run_shape("wide", args.wide_rows, 100)
torch.cuda.empty_cache()
run_shape("short", args.short_rows, 8)
if args.json:
    with open(args.json, "w") as f:
        json.dump(results, f, indent=1)
ctx.close()
