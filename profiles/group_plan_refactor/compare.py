"""Two builds of libchq.so against each other for the group filter's split into host plans, concatenations and orchestration:
`--before` is a build of the parent commit (same ABI, loaded through CHQ_LIB_PATH), the build in the tree is "after".  Every
measurement is a process of its own per build, under its own `timeout`; nothing more is started after a failure.

    python profiles/group_plan_refactor/compare.py --before OLD/libchq.so --outputs --out before_after.json
        the group shapes of the GPU suites, host and device resident, host and device results, per batch and coalesced, under
        the options group_fold, group_bits, group_mode, tile_kind, group_chunk_bytes and uniform_utf8_rows: a SHA-256 per call
        over the results and the call's chq_call_stats, or the error's code and message, under both builds, which must be equal
    python profiles/group_plan_refactor/compare.py --before OLD/libchq.so --launches --out launches.json
        one rocprofv3 --kernel-trace --memory-copy-trace run per build (no counters) of a 2000-batch device group of the
        reference schema and the same group host-resident: the multiset of (kernel, grid, block) and the copies per direction,
        which must be equal
    python profiles/group_plan_refactor/compare.py --before OLD/libchq.so --runs 3 --out before_after.json
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
STATS = ("rows_in", "rows_out", "tiles", "launches", "bytes_read_alg", "bytes_written_alg")


# ---- what runs under one build (child processes of this script) -----------------------------------------------------------------
def column_digest(col) -> str:
    """SHA-256 over one host column as its reader sees it (Arrow slice offsets applied): the validity, then the values
    (Boolean: the bits; fixed width: the bytes, zero where null; Utf8: the lengths' running sum and the string bytes)"""
    import numpy as np
    import pyarrow as pa
    n, off = len(col), col.offset
    h = hashlib.sha256(f"{col.type} {n} {col.null_count}|".encode())
    if n == 0:
        return h.hexdigest()
    valid = col.is_valid().to_numpy(zero_copy_only=False)
    h.update(np.packbits(valid, bitorder="little").tobytes())
    bufs = col.buffers()
    if pa.types.is_string(col.type):
        o = np.frombuffer(bufs[1], dtype=np.int32)[off:off + n + 1]
        h.update((o - o[0]).tobytes())
        h.update(bytes(memoryview(bufs[2])[int(o[0]):int(o[-1])]) if bufs[2] is not None else b"")
    elif pa.types.is_boolean(col.type):
        h.update(np.packbits(col.fill_null(False).to_numpy(zero_copy_only=False), bitorder="little").tobytes())
    else:
        w = col.type.bit_width // 8
        v = np.frombuffer(bufs[1], dtype=np.uint8)[off * w:(off + n) * w].reshape(n, w).copy()
        v[~valid] = 0
        h.update(v.tobytes())
    return h.hexdigest()


def batch_digest(b) -> str:
    return hashlib.sha256("".join(column_digest(c) for c in b.columns).encode()).hexdigest()


def group_cases():
    """name -> (batches, predicates): the shapes of tests/test_gpu_group.py, test_gpu_utf8_fold.py and test_gpu_views.py"""
    import numpy as np
    import pyarrow as pa

    def fixed(n, seed, wide=True):
        r = np.random.default_rng(seed)
        cols = {"id": pa.array(r.integers(-10**6, 10**6, n).astype(np.int32)), "value1": pa.array((r.random(n) * 40 - 10).astype(np.float32)),
                "value2": pa.array((r.random(n) * 40 - 10).astype(np.float32)), "b": pa.array(r.integers(-128, 128, n).astype(np.int8)),
                "h": pa.array(r.integers(0, 65536, n).astype(np.uint16))}
        if wide:
            cols["big"] = pa.array(r.integers(-10**12, 10**12, n).astype(np.int64))
            cols["d"] = pa.array(r.random(n) * 100)
        return pa.record_batch(cols)

    def nullable(b, rows, seed):
        r = np.random.default_rng(seed + b)
        n = rows - int(r.integers(0, 40))
        m = (lambda p: r.random(n) < p) if b % 3 != 1 else (lambda p: None)      # every third batch carries no bitmap at all
        return pa.RecordBatch.from_arrays([
            pa.array(r.integers(-1000, 1000, n).astype(np.int32), mask=m(0.2)), pa.array((r.random(n) * 100).astype(np.float32), mask=m(0.05)),
            pa.array(r.integers(0, 2, n).astype(bool), mask=m(0.3)), pa.array(r.integers(0, 2, n).astype(bool)),
            pa.array(r.integers(-2**40, 2**40, n), type=pa.int64(), mask=m(0.5)), pa.array(["s%d" % v for v in r.integers(0, 50, n)]),
            pa.array(r.integers(0, 200, n).astype(np.uint8))], names=["a", "x", "flag", "flag2", "big", "name", "tiny"])

    def strings(n, seed, two, longest=20, nulls=False):
        r = np.random.default_rng(seed)
        cols = {"id": pa.array(r.integers(0, 1000, n).astype(np.int32)),
                "s": pa.array(["w" * int(l) + str(i % 7) for i, l in enumerate(r.integers(0, longest, n))], mask=(r.random(n) < 0.1) if nulls else None),
                "v": pa.array((r.random(n) * 100).astype(np.float32))}
        if two:
            cols["t"] = pa.array(["%x" % v for v in r.integers(0, 2**31, n)])
            cols["k"] = pa.array(r.integers(-9, 9, n).astype(np.int64))
        return pa.record_batch(cols)

    def uniform(n, seed):
        r = np.random.default_rng(seed)
        return pa.record_batch({"id": pa.array(r.integers(0, 1000, n).astype(np.int32)), "key": pa.array(["%08x" % v for v in r.integers(0, 2**32, n)]),
                                "v": pa.array((r.random(n) * 100).astype(np.float32))})

    ragged = [2, 3, 63, 64, 65, 2047, 2048, 2049, 10_000, 16_383, 16_384, 16_385, 40_000, 5]
    sliced = [nullable(b, 3000, 50) for b in range(9)]
    sliced[4] = sliced[4].slice(3, sliced[4].num_rows - 7)          # Arrow offsets: bitmaps start mid-byte
    return {
        "fixed ragged": ([fixed(n, 100 + i) for i, n in enumerate(ragged)], ["value2 > 10.0", "big / 3 > h or d * 2.0 < 50.0", "id <> id"]),
        "fixed near-uniform": ([fixed(n, 300 + i) for i, n in enumerate([10_000] * 9 + [3333, 10_000, 9_999, 2])], ["value2 > 10.0", "id % 2 = 0 and value1 < 20.0"]),
        "fixed 1025 x 3": ([fixed(1025, 400 + i, False) for i in range(3)], ["value2 > 10.0"]),
        "fixed with a short batch": ([fixed(n, 560 + n) for n in (100, 0, 1, 5000)], ["value2 > 10.0"]),
        "fixed, error in batch 2": ([fixed(n, 600 + n) for n in (3000, 3001, 3002)], ["100 / b > 1", "nope > 1"]),
        "nullable, Boolean, Utf8": ([nullable(b, 10_000, 10) for b in range(9)], ["tiny > 100", "a + 1 > 0 and x < 50.0", "flag = flag2 or a < 5", "big > 0 and flag2"]),
        "nullable, sliced": (sliced, ["a > 0", "flag"]),
        "short strings, one column": ([strings(10_000, 500 + i, False) for i in range(12)], ["v > 10.0", "id < 0", "s >= 'ww'"]),
        "short strings, two columns, ragged": ([strings(n, 520 + i, True) for i, n in enumerate([70_000, 3, 16_384, 16_385, 2, 50_000])], ["v > 10.0", "id % 2 = 0"]),
        "short strings with nulls": ([strings(4000, 540 + i, False, nulls=True) for i in range(6)], ["v > 10.0"]),
        "long strings": ([strings(3000, 560 + i, False, longest=120) for i in range(5)], ["v > 10.0"]),
        "uniform-length strings": ([uniform(5000, 580 + i) for i in range(8)], ["v > 10.0", "id % 2 = 0"]),
    }


OPTION_SETS = [{}, {"group_fold": 0}, {"group_bits": 0}, {"group_mode": 1}, {"group_mode": 2}, {"tile_kind": 0}, {"tile_kind": 1, "group_mode": 2},
               {"group_chunk_bytes": 20_000}, {"group_chunk_bytes": 200_000, "group_fold": 0}, {"uniform_utf8_rows": 1}, {"uniform_utf8_rows": 1, "group_chunk_bytes": 100_000}]


def child_outputs():
    import chapterhouseqe_amd as chq
    from chapterhouseqe_amd.sqlparse import parse_expr
    out = {}
    for name, (recs, predicates) in group_cases().items():
        al = [[] for _ in recs[0].schema.names]
        for options in OPTION_SETS:
            ctx = chq.Context(0)
            for k, v in options.items():
                ctx.set_option(k, v)
            devs = [chq.DeviceRecordBatch.from_host(r, ctx) for r in recs]
            for sql in predicates:
                e = parse_expr(sql)
                for resident, src in (("host", recs), ("device", devs)):
                    for device_result in (False, True):
                        for coalesced in (False, True):
                            key = f"{name} | {json.dumps(options, sort_keys=True)} | {sql} | {resident} in | {'device' if device_result else 'host'} out | {'coalesced' if coalesced else 'per batch'}"
                            try:
                                if coalesced:
                                    big, per = chq.filter_records_coalesced(src, al, e, ctx=ctx, device_result=device_result)
                                    got, extra = [big], per
                                else:
                                    got, extra = chq.filter_records(src, al, e, ctx=ctx, device_result=device_result), None
                                st = ctx.last_stats()
                                got = [g.to_host() if device_result else g for g in got]
                                out[key] = {"stats": {k: int(st[k]) for k in STATS}, "rows_per_batch": extra, "batches": [batch_digest(g) for g in got]}
                            except chq.ChqError as err:
                                out[key] = {"error": [err.code, err.message]}
            ctx.close()
    print(json.dumps(out))


def reference_group(nb=2000, rows=10_000):
    """bench/micro/group_host.py's table: id:i32, value1:Utf8(8), value2:f32 in `nb` batches of `rows` rows"""
    import numpy as np
    import pyarrow as pa
    rng = np.random.default_rng(7)
    n = nb * rows
    chars = rng.integers(ord("a"), ord("z") + 1, n * 8, dtype=np.uint8)
    offs = (np.arange(n + 1, dtype=np.int64) * 8).astype(np.int32)
    strs = pa.Array.from_buffers(pa.utf8(), n, [None, pa.py_buffer(offs.tobytes()), pa.py_buffer(chars.tobytes())])
    full = pa.RecordBatch.from_arrays([pa.array(np.arange(n, dtype=np.int32)), strs, pa.array((rng.random(n) * 100).astype(np.float32))], names=["id", "value1", "value2"])
    return [full.slice(b * rows, rows) for b in range(nb)]


def child_trace():
    import chapterhouseqe_amd as chq
    from chapterhouseqe_amd.sqlparse import parse_expr
    ctx = chq.Context(0)
    recs = reference_group()
    e = parse_expr("value2 > 10.0")
    devs = [chq.DeviceRecordBatch.from_host(r, ctx) for r in recs]
    out = {}
    for name, src in (("device", devs), ("host", recs)):
        got = chq.filter_records(src, [[], [], []], e, ctx=ctx, device_result=False)
        st = ctx.last_stats()
        out[name] = {"stats": {k: int(st[k]) for k in STATS}, "sha256": hashlib.sha256("".join(batch_digest(g) for g in got).encode()).hexdigest()}
    ctx.close()
    print(json.dumps(out))


def child_large():
    """the 12 500-batch call of tests/test_gpu_group.py::test_large_group_many_small_batches, timed around the call"""
    import torch
    import chapterhouseqe_amd as chq
    from chapterhouseqe_amd.sqlparse import parse_expr
    ctx = chq.Context(0)
    nb, rows = 12_500, 10_000
    g = torch.Generator(device="cuda").manual_seed(3)
    cols = [torch.rand(nb * rows, generator=g, device="cuda", dtype=torch.float32) * 20.0 for _ in range(3)]
    torch.cuda.synchronize()
    devs = [chq.DeviceRecordBatch.from_device_pointers([(name, "f", c.data_ptr() + 4 * b * rows) for name, c in zip(("id", "value1", "value2"), cols)], rows, ctx)
            for b in range(nb)]
    grp = chq.RecordGroup(devs, ctx)
    e = parse_expr("value2 > 10.0")
    times = []
    for _ in range(12):
        t0 = time.perf_counter()
        counts = chq.filter_records(grp, [[], [], []], e, ctx=ctx, wrap=False)
        times.append((time.perf_counter() - t0) * 1e3)
    assert sum(counts) == int((cols[2] > 10.0).sum()) and ctx.last_stats()["launches"] == 1
    print(json.dumps({"call_ms": statistics.median(times[2:])}))


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
    result = {"calls": len(names), "of_which_errors": errors, "differing": differing, "sha256_of_all": digest,
              "differing_cases": {n: {"before": got["before"].get(n), "after": got["after"].get(n)} for n in differing},
              "error_counts": {}, "launches_histogram": {}}
    for n in names:          # (which calls end in which error, and every call's stats, are in `sha256_of_all`; here how many of each)
        r = got["after"].get(n) or {}
        if "error" in r:
            code, message = r["error"]
            result["error_counts"][f"{code} {message}"] = result["error_counts"].get(f"{code} {message}", 0) + 1
        elif "stats" in r:
            k = str(r["stats"]["launches"])
            result["launches_histogram"][k] = result["launches_histogram"].get(k, 0) + 1
    print(f"{len(names)} calls ({errors} of them errors), {len(differing)} differ", *differing[:20], sep="\n  ")
    return result, not differing


def read_trace(directory):
    def rows(pattern):
        out = []
        for path in glob.glob(os.path.join(directory, "**", pattern), recursive=True):
            with open(path, newline="") as f:
                out += list(csv.DictReader(f))
        return sorted(out, key=lambda r: int(r["Start_Timestamp"]))
    kernels = [{"kernel": r["Kernel_Name"], "grid": [int(r["Grid_Size_" + d]) for d in "XYZ"], "block": [int(r["Workgroup_Size_" + d]) for d in "XYZ"]}
               for r in rows("*kernel_trace.csv")]
    copies = {}
    for r in rows("*memory_copy_trace.csv"):
        copies[r["Direction"]] = copies.get(r["Direction"], 0) + 1
    return {"kernels": kernels, "copies": copies}


def launches(args):
    got = {}
    for build in ("before", "after"):
        with tempfile.TemporaryDirectory() as d:
            text = run(["rocprofv3", "--kernel-trace", "--memory-copy-trace", "--output-format", "csv", "-d", d, "-o", "trace", "--",
                        sys.executable, __file__, "--child", "trace"], 280, build, args.before)
            got[build] = read_trace(d)
            got[build]["outputs"] = last_json(text)
    key = lambda k: json.dumps([k["kernel"], k["grid"], k["block"]])
    shape = {b: {"launches": sorted(key(k) for k in got[b]["kernels"]), "copies": got[b]["copies"]} for b in got}
    verdict = {k: shape["before"][k] == shape["after"][k] for k in shape["after"]}
    verdict["outputs"] = got["before"]["outputs"] == got["after"]["outputs"]
    same = all(verdict.values()) and len(got["after"]["kernels"]) > 0
    counts = {}
    for k in got["after"]["kernels"]:
        counts[k["kernel"].split("(")[0]] = counts.get(k["kernel"].split("(")[0], 0) + 1
    print(f"{len(got['before']['kernels'])} launches before, {len(got['after']['kernels'])} after; copies {got['before']['copies']} / {got['after']['copies']}: {verdict}")
    result = {"equal": same, "verdict": verdict, "launches": len(got["after"]["kernels"]), "kernel_counts": counts, "copies": got["after"]["copies"],
              "calls": got["after"]["outputs"],
              "sha256_of_shape": {b: hashlib.sha256(json.dumps(shape[b], sort_keys=True).encode()).hexdigest() for b in shape}}
    if not same:             # (the launches themselves are kept only where they have to be looked at)
        result["kernels"] = {build: got[build]["kernels"] for build in got}
    return result, same


def parse_bench(text):
    j = last_json(text)
    return {"headline (ms/step)": j["ms_per_step"], "config5_shard.call_ms": j["extra"]["config5_shard"]["call_ms"]} if "config5_shard" in j.get("extra", {}) \
        else {"headline (ms/step)": j["ms_per_step"]}


def parse_group_host(text):
    return {f"{m.group(1)}: filter_records (ms)": float(m.group(2)) for m in re.finditer(r"^(\w+) \(.*?\| one group call ([\d.]+) ms", text, re.M)}


BENCHES = {   # name -> (command, seconds allowed, parser); lower is better
    "bench": ([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5", "--no-cpu-baseline"], 500, parse_bench),
    "group_host": ([sys.executable, "bench/micro/group_host.py"], 300, parse_group_host),
    "large_group": ([sys.executable, os.path.relpath(__file__, ROOT), "--child", "large"], 200, lambda text: {"12 500 x 10 000 rows, one call (ms)": last_json(text)["call_ms"]}),
}


def timing(args):
    result = {"runs_per_build": args.runs, "order": "before, after, before, after, ...", "lines": {}}
    for name in args.only or list(BENCHES):
        cmd, limit, parse = BENCHES[name]
        raw = {"before": {}, "after": {}}
        for _ in range(args.runs):
            for build in ("before", "after"):
                for key, value in parse(run(cmd, limit, build, args.before)).items():
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
    ap.add_argument("--child", choices=["outputs", "trace", "large"], help=argparse.SUPPRESS)
    ap.add_argument("--before", help="libchq.so of the build to compare against")
    ap.add_argument("--outputs", action="store_true")
    ap.add_argument("--launches", action="store_true")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--only", action="append", choices=sorted(BENCHES), default=None)
    ap.add_argument("--key", default=None, help="entry of the output file (default: outputs / launches / three_runs)")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.child:
        return {"outputs": child_outputs, "trace": child_trace, "large": child_large}[args.child]()
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
