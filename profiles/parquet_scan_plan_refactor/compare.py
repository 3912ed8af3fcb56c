"""Two builds of libchq.so against each other for the Parquet scan's split into host plans and orchestration: `--before` is a
build of the parent commit (same ABI, loaded through CHQ_LIB_PATH), the build in the tree is "after".  Every measurement is a
process of its own per build, under its own `timeout`; nothing more is started after a failure.

    python profiles/parquet_scan_plan_refactor/compare.py --before OLD/libchq.so --outputs --out before_after.json
        every file of tests/parquet_plan_files.py (the pyarrow-written set, both forged suites, the files the host refuses),
        from memory and through a range reader, with all columns and with a pruned column list: a SHA-256 over each decoded
        column's buffers, or the error's code and message, under both builds, which must be equal
    python profiles/parquet_scan_plan_refactor/compare.py --before OLD/libchq.so --launches --out launches.json
        one rocprofv3 --kernel-trace --memory-copy-trace run per build (no counters) of a 20-row-group snappy scan and an
        uncompressed scan: the multiset of (kernel, grid, block), the order per stream and the copies per direction, which
        must be equal
    python profiles/parquet_scan_plan_refactor/compare.py --before OLD/libchq.so --runs 3 --out before_after.json
        host time, the builds alternating: a line passes when the new build's median lies inside the old build's own
        min..max over its runs (`--only` picks benchmarks; `--key` names the entry of the output file)
"""
import argparse
import csv
import glob
import hashlib
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


# ---- what runs under one build (child processes of this script) -----------------------------------------------------------------
def column_digest(col) -> str:
    """SHA-256 over the buffers of one host column cut to their logical lengths: validity bits (padding bits cleared), then the
    values (Boolean: bits; fixed width: the bytes, zero where null; Utf8: offsets and string bytes)"""
    import numpy as np
    import pyarrow as pa
    n = len(col)
    h = hashlib.sha256(f"{col.type} {n} {col.null_count}|".encode())
    bufs = col.buffers()
    assert col.offset == 0
    if n == 0:
        return h.hexdigest()

    def bits(buf):
        b = np.frombuffer(buf, dtype=np.uint8, count=(n + 7) // 8).copy()
        if n % 8:
            b[-1] &= (1 << (n % 8)) - 1
        return b
    valid = np.unpackbits(bits(bufs[0]), bitorder="little")[:n].astype(bool) if bufs[0] is not None and col.null_count else np.ones(n, dtype=bool)
    h.update(np.packbits(valid, bitorder="little").tobytes())
    if pa.types.is_string(col.type):
        offsets = np.frombuffer(bufs[1], dtype=np.int32, count=n + 1)
        h.update(offsets.tobytes())
        h.update(bytes(memoryview(bufs[2])[:int(offsets[-1])]) if bufs[2] is not None else b"")
    elif pa.types.is_boolean(col.type):
        h.update((bits(bufs[1]) & np.packbits(valid, bitorder="little")).tobytes())
    else:
        w = col.type.bit_width // 8
        v = np.frombuffer(bufs[1], dtype=np.uint8, count=n * w).reshape(n, w).copy()
        v[~valid] = 0
        h.update(v.tobytes())
    return h.hexdigest()


def child_outputs():
    import chapterhouseqe_amd as chq
    from tests import parquet_plan_files as PF

    files = {**PF.pyarrow_files(), **PF.forged_files(), **{n: v[0] for n, v in PF.host_refused().items()}}
    ctx = chq.Context(0)
    out = {}
    for name, raw in files.items():
        for source in ("memory", "reader"):
            for pruned in (False, True):
                key = f"{name} | {source} | {'pruned' if pruned else 'all columns'}"
                try:
                    f = chq.ParquetFile(raw) if source == "memory" else chq.ParquetFile(None, reader=lambda off, ln, raw=raw: raw[off:off + ln], size=len(raw))
                    columns = list(range(f.num_columns))[::-2] if pruned else None      # (every other column, the last one first)
                    got = f.read_row_groups(ctx=ctx, columns=columns)
                    out[key] = {"stats": {k: int(v) for k, v in ctx.last_stats().items() if k in ("rows_in", "rows_out", "bytes_read_alg", "bytes_written_alg")},
                                "row_groups": [[column_digest(c) for c in b.to_host().columns] for b in got]}
                    f.close()
                except chq.ChqError as e:
                    out[key] = {"error": [e.code, e.message]}
    ctx.close()
    print(json.dumps(out))


def trace_files():
    import numpy as np
    import pyarrow as pa
    from tests.parquet_cases import write_bytes
    n = 20 * 50_000
    rng = np.random.default_rng(3)
    t = pa.table({"id": pa.array(np.arange(n, dtype=np.int32)), "value1": pa.array(["%08x" % v for v in rng.integers(0, 2**32, n)]),
                  "value2": pa.array((rng.random(n) * 100).astype(np.float32), mask=rng.random(n) < 0.1)})
    return {codec: write_bytes(t, compression=codec, row_group_size=50_000) for codec in ("snappy", "none")}


def child_trace():
    import chapterhouseqe_amd as chq
    ctx = chq.Context(0)
    out = {}
    for codec, raw in trace_files().items():
        f = chq.ParquetFile(raw)
        got = f.read_row_groups(ctx=ctx)
        assert len(got) == 20
        out[codec] = hashlib.sha256("".join(column_digest(c) for b in got for c in b.to_host().columns).encode()).hexdigest()
        f.close()
    ctx.close()
    print(json.dumps(out))


# ---- the parent ----------------------------------------------------------------------------------------------------------------------
def run(cmd, limit, build, before):
    """one process under `timeout`; its stdout"""
    env = dict(os.environ)
    env.pop("CHQ_LIB_PATH", None)
    if build == "before":
        env["CHQ_LIB_PATH"] = os.path.abspath(before)
    done = subprocess.run(["timeout", "-k", "10", str(limit), *cmd], cwd=ROOT, env=env, capture_output=True, text=True)
    if done.returncode != 0:   # nothing more is started after a failure
        sys.exit(f"{' '.join(cmd)} ({build}) exited with {done.returncode}:\n{done.stdout[-2000:]}\n{done.stderr[-4000:]}")
    return done.stdout


def last_json(text):
    return json.loads([ln for ln in text.splitlines() if ln.startswith("{")][-1])


def outputs(args):
    got = {build: last_json(run([sys.executable, __file__, "--child", "outputs"], 500, build, args.before)) for build in ("before", "after")}
    names = sorted(set(got["before"]) | set(got["after"]))
    differing = [n for n in names if got["before"].get(n) != got["after"].get(n)]
    errors = sum(1 for n in names if "error" in (got["after"].get(n) or {}))
    digest = {b: hashlib.sha256(json.dumps(got[b], sort_keys=True).encode()).hexdigest() for b in got}
    result = {"reads": len(names), "of_which_errors": errors, "differing": differing, "sha256_of_all": digest,
              "differing_cases": {n: {"before": got["before"].get(n), "after": got["after"].get(n)} for n in differing},
              "error_counts": {}}
    for n in names:          # (which reads end in which error is in `sha256_of_all`; here how many of each)
        if "error" in (got["after"].get(n) or {}):
            code, message = got["after"][n]["error"]
            result["error_counts"][f"{code} {message}"] = result["error_counts"].get(f"{code} {message}", 0) + 1
    print(f"{len(names)} reads ({errors} of them errors), {len(differing)} differ", *differing, sep="\n  ")
    return result, not differing


def read_trace(directory):
    def rows(pattern):
        out = []
        for path in glob.glob(os.path.join(directory, "**", pattern), recursive=True):
            with open(path, newline="") as f:
                out += list(csv.DictReader(f))
        return sorted(out, key=lambda r: int(r["Start_Timestamp"]))
    launches = rows("*kernel_trace.csv")
    by = next((k for k in ("Stream_Id", "Queue_Id") if launches and k in launches[0]), None)
    kernels = [{"kernel": r["Kernel_Name"], "grid": [int(r["Grid_Size_" + d]) for d in "XYZ"], "block": [int(r["Workgroup_Size_" + d]) for d in "XYZ"],
                "stream": r.get(by)} for r in launches]
    copies = {}
    for r in rows("*memory_copy_trace.csv"):
        copies[r["Direction"]] = copies.get(r["Direction"], 0) + 1
    return {"kernels": kernels, "copies": copies, "streams_by": by}


def shape(trace):
    """what must be equal: the multiset of (kernel, grid, block); the launch sequence of every stream (the streams' ids are the
    runtime's: the sequences are compared as a multiset); the copies per direction"""
    key = lambda k: json.dumps([k["kernel"], k["grid"], k["block"]])
    per_stream = {}
    for k in trace["kernels"]:
        per_stream.setdefault(k["stream"], []).append(key(k))
    return {"launches": sorted(key(k) for k in trace["kernels"]), "per_stream": sorted(per_stream.values()), "copies": trace["copies"]}


def launches(args):
    got = {}
    for build in ("before", "after"):
        with tempfile.TemporaryDirectory() as d:
            text = run(["rocprofv3", "--kernel-trace", "--memory-copy-trace", "--output-format", "csv", "-d", d, "-o", "trace", "--",
                        sys.executable, __file__, "--child", "trace"], 280, build, args.before)
            got[build] = read_trace(d)
            got[build]["outputs"] = last_json(text)
    a, b = shape(got["before"]), shape(got["after"])
    verdict = {k: a[k] == b[k] for k in a}
    verdict["outputs"] = got["before"]["outputs"] == got["after"]["outputs"]
    same = all(verdict.values()) and len(got["after"]["kernels"]) > 0
    counts = {}
    for k in got["after"]["kernels"]:
        counts[k["kernel"].split("(")[0]] = counts.get(k["kernel"].split("(")[0], 0) + 1
    print(f"{len(got['before']['kernels'])} launches before, {len(got['after']['kernels'])} after on {len(b['per_stream'])} streams (by {got['after']['streams_by']}); "
          f"copies {got['before']['copies']} / {got['after']['copies']}: {verdict}")
    result = {"equal": same, "verdict": verdict, "launches": len(got["after"]["kernels"]), "streams": len(b["per_stream"]), "streams_by": got["after"]["streams_by"],
              "launches_per_stream": sorted(len(q) for q in b["per_stream"]), "kernel_counts": counts, "copies": got["after"]["copies"],
              "sha256_of_shape": {"before": hashlib.sha256(json.dumps(a, sort_keys=True).encode()).hexdigest(),
                                  "after": hashlib.sha256(json.dumps(b, sort_keys=True).encode()).hexdigest()}}
    if not same:             # (the launches themselves are kept only where they have to be looked at)
        result["kernels"] = {build: got[build]["kernels"] for build in got}
    return result, same


def parse_parquet_scan(text):
    one = re.search(r"chq scan \(metadata .*?one call\): ([\d.]+) ms", text)
    each = re.search(r"chq scan, one call per row group: ([\d.]+) ms", text)
    return {"scan, one call (ms)": float(one.group(1)), "scan, one call per row group (ms)": float(each.group(1))}


def parse_ragged(text):
    return {f"ragged strings, use_dictionary={m.group(1)}: scan (ms)": float(m.group(2)) for m in re.finditer(r"use_dictionary=(\w+):.*?chq scan ([\d.]+) ms", text)}


def parse_bench(text):
    return {"headline (ms/step)": last_json(text)["ms_per_step"]}


BENCHES = {   # name -> (command, seconds allowed, parser or None = the process's wall time, runs per build or None = --runs); lower is better
    "parquet_scan": ([sys.executable, "bench/micro/parquet_scan.py", "8000000", "none"], 400, parse_parquet_scan, None),
    "parquet_scan_snappy": ([sys.executable, "bench/micro/parquet_scan.py", "8000000", "snappy"], 400, parse_parquet_scan, None),
    "parquet_ragged": ([sys.executable, "bench/micro/parquet_ragged.py"], 400, parse_ragged, None),
    "snappy_pages": ([sys.executable, "bench/micro/snappy_pages.py"], 300, None, None),
    "bench": ([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5", "--no-cpu-baseline", "--no-extra"], 400, parse_bench, 2),
}


def timing(args):
    result = {"runs_per_build": args.runs, "order": "before, after, before, after, ...", "lines": {}}
    for name in args.only or list(BENCHES):
        cmd, limit, parse, runs = BENCHES[name]
        raw = {"before": {}, "after": {}}
        for _ in range(runs or args.runs):
            for build in ("before", "after"):
                t0 = time.perf_counter()
                text = run(cmd, limit, build, args.before)
                figures = parse(text) if parse else {"process wall time (s)": round(time.perf_counter() - t0, 2)}
                for key, value in figures.items():
                    raw[build].setdefault(key, []).append(value)
                print(name, build, "done", flush=True)
        for key in raw["before"]:
            before, after = raw["before"][key], raw["after"][key]
            med = statistics.median(after)
            verdict = "inside" if min(before) <= med <= max(before) else ("outside: faster" if med < min(before) else "outside: slower")
            result["lines"][f"{name}: {key}"] = {
                "command": " ".join(cmd[1:]), "before": before, "after": after, "before_min": min(before), "before_max": max(before),
                "before_median": statistics.median(before), "after_median": med, "verdict": verdict}
            print(f"{name}: {key}: before {min(before):.4g}..{max(before):.4g} (median {statistics.median(before):.4g}), "
                  f"after median {med:.4g}: {verdict}", flush=True)
    return result, True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=["outputs", "trace"], help=argparse.SUPPRESS)
    ap.add_argument("--before", help="libchq.so of the build to compare against")
    ap.add_argument("--outputs", action="store_true")
    ap.add_argument("--launches", action="store_true")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--only", action="append", choices=sorted(BENCHES), default=None)
    ap.add_argument("--key", default=None, help="entry of the output file (default: outputs / launches / three_runs)")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.child:
        return child_outputs() if args.child == "outputs" else child_trace()
    if not args.before or not args.out:
        ap.error("--before and --out are required")
    mode, key = (outputs, "outputs") if args.outputs else (launches, "launches") if args.launches else (timing, "three_runs")
    result, ok = mode(args)
    merged = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            merged = json.load(f)
    merged[args.key or key] = result
    with open(args.out, "w") as f:
        json.dump(merged, f, indent=1)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
