"""Scalar string functions on a device-resident batch of the reference's sample shape (id: Int32,
value1: Utf8 of random lower-case letters, value2: Float32), in the two shapes of bench/micro/like.py:

  wide    20 M rows x 100-byte value1: strfn.hip's wave-per-row mode
  short   100 M rows x 8-byte value1: lane per row throughout

Timed, with the host clock around the call (the temporary column's kernels, its read-backs, and the export of the result):

  select upper(value1)                      the byte map + the rebased offsets
  select value1 || '-' || value1            row lengths, scan, gather from three parts (on the wide shape over the first
                                            10 M rows: 20 M results of 201 bytes pass the Int32 offset range)
  select substring(value1 from 2 for 3)     row windows, scan, gather from one range
  where length(value1) > 3                  filter_record: the Int32 temporary, the filter kernel that reads it, the copy of
                                            the surviving rows (all of them: every value has more than 3 characters)

GB/s = (offsets + string data of value1) read per second.  Two lines to measure against, in the same run on the same batch:

  copy              torch.clone of value1's offsets and data buffers: the ceiling for the byte map, which reads and writes
                    the same bytes
  host              pyarrow.compute (ascii_upper, binary_join_element_wise, utf8_slice_codeunits, utf8_length) over the
                    first --host-rows rows of the same column

usage: python bench/micro/strfn.py [--wide-rows N] [--short-rows N] [--host-rows N] [--reps R] [--json PATH]"""
import argparse
import json
import sys
import time

sys.path.insert(0, ".")
import chapterhouseqe_amd as chq   # noqa: E402
from chapterhouseqe_amd.sqlparse import parse_expr, parse_select   # noqa: E402

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
ALIASES = [[]] * 3
SELECTS = ["upper(value1)", "value1 || '-' || value1", "substring(value1 from 2 for 3)"]
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

    def report(label, seconds, rows_out=None, rows=n, read=nbytes):
        r = {"shape": name, "rows": rows, "width": width, "what": label, "rows_out": rows_out, "ms": seconds * 1e3, "GBps": read / seconds / 1e9}
        results.append(r)
        print(f"  {label:44s} {r['ms']:10.3f} ms {r['GBps']:9.1f} GB/s", flush=True)
        return r

    def project(fields):
        out = chq.project_record(fields, rec, ALIASES, ctx=ctx)
        out.release()

    def filt(e):
        out = chq.filter_record(rec, ALIASES, e, ctx=ctx)
        rows = out.num_rows
        out.release()
        return rows

    def clone():
        a, b = offs.clone(), letters.clone()
        torch.cuda.synchronize()
        del a, b

    copy = report("copy (torch.clone of offsets + data)", best_of(clone))
    for sql in SELECTS:
        fields = parse_select(f"select {sql} from t").projection
        if "||" in sql and n * (2 * width + 1) > 2**31 - 1:
            # the result would pass the Int32 offset range (the library says so): the first rows that fit, whole millions
            m = (2**31 - 1) // (2 * width + 1) // 1_000_000 * 1_000_000
            part = rec.slice(0, m)

            def project_part():
                out = chq.project_record(fields, part, ALIASES, ctx=ctx)
                out.release()
            report(f"select {sql} (first {m} rows)", best_of(project_part), rows=m, read=4 * (m + 1) + m * width)
            continue
        r = report(f"select {sql}", best_of(lambda: project(fields)))
        if sql.startswith("upper"):
            r["fraction_of_copy"] = copy["ms"] / r["ms"]
            print(f"    = {r['fraction_of_copy']:.2f} of the copy line", flush=True)
    e = parse_expr("length(value1) > 3")
    report("where length(value1) > 3", best_of(lambda: filt(e)), rows_out=filt(e))
    # the host lines: the first host_rows rows of the same column
    m = min(n, args.host_rows)
    harr = pa.Array.from_buffers(pa.utf8(), m, [None, pa.py_buffer(offs[: m + 1].cpu().numpy().tobytes()), pa.py_buffer(letters[: m * width].cpu().numpy().tobytes())])
    hbytes = 4 * (m + 1) + m * width
    for label, fn in (("host ascii_upper", lambda: pc.ascii_upper(harr)), ("host binary_join_element_wise", lambda: pc.binary_join_element_wise(harr, pa.scalar("-"), harr, "")),
                      ("host utf8_slice_codeunits(1, 4)", lambda: pc.utf8_slice_codeunits(harr, 1, 4)), ("host utf8_length > 3", lambda: pc.greater(pc.utf8_length(harr), 3))):
        t0 = time.perf_counter()
        fn()
        report(f"{label} on {m} rows", time.perf_counter() - t0, rows=m, read=hbytes)
    rec.release()


run_shape("wide", args.wide_rows, 100)
torch.cuda.empty_cache()
run_shape("short", args.short_rows, 8)
if args.json:
    with open(args.json, "w") as f:
        json.dump(results, f, indent=1)
ctx.close()
