"""Two builds of libchq.so against each other for the Parquet writer's split into device encode, layout and assembly:
`--before` is a build of the parent commit (same ABI, loaded through CHQ_LIB_PATH), the build in the tree is "after".
Every measurement is a process of its own per build, under its own `timeout`; nothing more is started after a failure.

    python profiles/parquet_write_refactor/compare.py --before OLD/libchq.so --images --out before_after.json
        every image of the page-encoder suite's batches (tests/parquet_write_cases.py), from a host and from a device batch,
        at parquet_page_rows 4096 and default: SHA-256 and length under both builds, which must be equal
    python profiles/parquet_write_refactor/compare.py --before OLD/libchq.so --launches --out launches.json
        one rocprofv3 --kernel-trace --memory-copy-trace run per build of two writes: the ordered kernel launches with grid
        and block sizes, and the copies per direction, which must be equal
    python profiles/parquet_write_refactor/compare.py --before OLD/libchq.so --runs 3 --out before_after.json
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

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


# ---- what runs under one build (child processes of this script) -----------------------------------------------------------------
def child_images():
    import chapterhouseqe_amd as chq
    from tests import parquet_write_cases as W

    def one_batch(t):
        return t.combine_chunks().to_batches()[0]

    cases = [("string_shapes", one_batch(W.string_shapes()), None)]        # (name, host source, (parent, offset) of a view or None)
    for shape, (valid, nullable, bitmap) in W.validity_shapes().items():
        cases.append((f"typed_batch {shape}", W.typed_batch(W.N, valid, nullable, seed=3, bitmap=bitmap), None))
    for offset in W.VIEW_OFFSETS:
        for shape in ("random_30", "page1_null", "no_nulls"):
            parent = W.view_parent(offset, shape)
            cases.append((f"view_parent {offset} {shape}", parent.slice(offset, W.N), (parent, offset)))
    cases.append(("statistics_cases", one_batch(W.statistics_cases()), None))
    for offset in W.STATS_VIEW_OFFSETS:
        parent = W.statistics_view_parent(offset)
        cases.append((f"statistics_view_parent {offset}", parent.slice(offset, W.N), (parent, offset)))
    groups = [(f"row_group_batches nullable={nullable}", W.row_group_batches(nullable)) for nullable in (True, False)]
    out = {}
    for page_rows in (4096, None):
        ctx = chq.Context(0)
        if page_rows:
            ctx.set_option("parquet_page_rows", page_rows)

        def note(name, who, raw):
            raw = bytes(raw)
            out[f"{name} | {who} | parquet_page_rows {page_rows or 'default'}"] = {"sha256": hashlib.sha256(raw).hexdigest(), "len": len(raw)}
        for name, host, view in cases:
            note(name, "host", chq.record_to_parquet(host, ctx=ctx))
            if view is None:
                dev = chq.DeviceRecordBatch.from_host(host, ctx=ctx)
                note(name, "device", chq.record_to_parquet(dev, ctx=ctx))
            else:
                dev = chq.DeviceRecordBatch.from_host(view[0], ctx=ctx)
                note(name, "device view", chq.record_to_parquet(dev.slice(view[1], W.N), ctx=ctx))
        for name, parts in groups:
            note(name, "host", chq.records_to_parquet(parts, ctx=ctx))
            note(name, "device", chq.records_to_parquet([chq.DeviceRecordBatch.from_host(p, ctx=ctx) for p in parts], ctx=ctx))
        ctx.close()
    print(json.dumps(out))


def child_trace():
    import chapterhouseqe_amd as chq
    from tests import parquet_write_cases as W

    ctx = chq.Context(0)
    ctx.set_option("parquet_page_rows", 4096)
    dev = chq.DeviceRecordBatch.from_host(W.typed_batch(W.N, W.thirty_percent(W.N), True, seed=3), ctx=ctx)
    a = bytes(chq.record_to_parquet(dev, ctx=ctx))
    b = bytes(chq.records_to_parquet(W.row_group_batches(True), ctx=ctx))
    ctx.close()
    print(json.dumps({"typed_batch": hashlib.sha256(a).hexdigest(), "row_groups": hashlib.sha256(b).hexdigest()}))


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


def images(args):
    got = {build: last_json(run([sys.executable, __file__, "--child", "images"], 500, build, args.before)) for build in ("before", "after")}
    names = sorted(set(got["before"]) | set(got["after"]))
    differing = [n for n in names if got["before"].get(n) != got["after"].get(n)]
    result = {"images": len(names), "differing": differing,
              "cases": {n: {"before": got["before"].get(n), "after": got["after"].get(n)} for n in names}}
    print(f"{len(names)} images, {len(differing)} differ", *differing, sep="\n  ")
    return result, not differing


def read_trace(directory):
    def rows(pattern):
        files = glob.glob(os.path.join(directory, "**", pattern), recursive=True)
        out = []
        for path in files:
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
            got[build]["images"] = last_json(text)
    same = got["before"] == got["after"] and len(got["after"]["kernels"]) > 0
    print(f"{len(got['before']['kernels'])} launches before, {len(got['after']['kernels'])} after; copies {got['before']['copies']} / {got['after']['copies']}: "
          + ("equal" if same else "DIFFERENT"))
    return {"equal": same, **got}, same


def parse_parquet_scan(text):
    m = re.search(r"chq record_to_parquet from a device batch .*?: ([\d.]+) ms", text)
    return {"record_to_parquet from a device batch (ms)": float(m.group(1))}


def parse_pipeline(text):
    m = re.search(r"stages: scan ([\d.]+) ms, filter \+ project ([\d.]+) ms, write ([\d.]+) ms", text)
    d = re.search(r"^device \(.*?\): (\d+) ms", text, re.M)
    return {"device: write stage (ms)": float(m.group(3)), "device: end to end (ms)": float(d.group(1))}


def parse_bench(text):
    line = last_json(text)
    out = {"headline (ms/step)": line["ms_per_step"]}
    pipeline = (line.get("extra") or {}).get("parquet_pipeline") or {}
    for key in ("call_ms", "write_ms"):
        if key in pipeline:
            out[f"parquet_pipeline {key}"] = pipeline[key]
    return out


BENCHES = {   # name -> (command, seconds allowed, parser, runs per build or None = --runs); every figure: lower is better
    "parquet_scan": ([sys.executable, "bench/micro/parquet_scan.py"], 400, parse_parquet_scan, None),
    "pipeline": ([sys.executable, "bench/micro/pipeline.py"], 400, parse_pipeline, None),
    "bench": ([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5", "--no-cpu-baseline", "--no-extra"], 400, parse_bench, 1),
}


def timing(args):
    result = {"runs_per_build": args.runs, "order": "before, after, before, after, ...", "lines": {}}
    for name in args.only or list(BENCHES):
        cmd, limit, parse, runs = BENCHES[name]
        raw = {"before": {}, "after": {}}
        for _ in range(runs or args.runs):
            for build in ("before", "after"):
                text = run(cmd, limit, build, args.before)
                for key, value in parse(text).items():
                    raw[build].setdefault(key, []).append(value)
                if name == "bench":
                    result.setdefault("bench roofline.traffic_source", {})[build] = last_json(text)["roofline"].get("traffic_source")
                print(name, build, "done", flush=True)
        for key in raw["before"]:
            before, after = raw["before"][key], raw["after"][key]
            med = statistics.median(after)
            verdict = "inside" if min(before) <= med <= max(before) else ("outside: faster" if med < min(before) else "outside: slower")
            if len(before) == 1:
                verdict = "one run per build: not judged"
            result["lines"][f"{name}: {key}"] = {
                "command": " ".join(cmd[1:]), "before": before, "after": after, "before_min": min(before), "before_max": max(before),
                "before_median": statistics.median(before), "after_median": med, "verdict": verdict}
            print(f"{name}: {key}: before {min(before):.4g}..{max(before):.4g} (median {statistics.median(before):.4g}), "
                  f"after median {med:.4g}: {verdict}", flush=True)
    return result, True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=["images", "trace"], help=argparse.SUPPRESS)
    ap.add_argument("--before", help="libchq.so of the build to compare against")
    ap.add_argument("--images", action="store_true")
    ap.add_argument("--launches", action="store_true")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--only", action="append", choices=sorted(BENCHES), default=None)
    ap.add_argument("--key", default=None, help="entry of the output file (default: images / launches / three_runs)")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.child:
        return child_images() if args.child == "images" else child_trace()
    if not args.before or not args.out:
        ap.error("--before and --out are required")
    mode, key = (images, "images") if args.images else (launches, "launches") if args.launches else (timing, "three_runs")
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
