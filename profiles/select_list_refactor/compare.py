"""Timing of two builds of libchq.so in ONE run, alternating: `--before` is another build of the same ABI (loaded through
CHQ_LIB_PATH), the build in the tree is "after".  Every benchmark runs `--runs` times per build as a process of its own, at
its default size (each warms itself up).  A line passes when the new build's median lies inside the old build's own
min..max over its runs.

    python profiles/select_list_refactor/compare.py --before /path/to/old/libchq.so --runs 3 --out before_after.json
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse_project_latency(text):
    return {f"n={m.group(1)} {m.group(2)} {m.group(3)} (us/call)": float(m.group(4))
            for m in re.finditer(r"n=\s*(\d+) (device|host)\s+(\w+)\s+([\d.]+) us/call", text)}


def parse_call_latency(text):
    return {f"n={m.group(1)} {m.group(2)} (us/call)": float(m.group(3))
            for m in re.finditer(r"n=\s*(\d+) (device|host)\s+([\d.]+) us/call", text)}


def parse_fused_probe(text):   # four iterations, the first one warms up: the best of the other three
    one = [(float(m.group(1)), float(m.group(2))) for m in re.finditer(r"one-pass \d+ launch ([\d.]+) ms kernel ([\d.]+) ms wall", text)][1:]
    two = [float(m.group(1)) for m in re.finditer(r"filter\+project wall ([\d.]+) ms", text)][1:]
    return {"one pass: kernel (ms)": min(k for k, _ in one), "one pass: wall (ms)": min(w for _, w in one),
            "two steps: wall (ms)": min(two)}


def parse_nullable_projection(text):
    out = {}
    for m in re.finditer(r"column a (with 6 % nulls|non-null): project_record ([\d.]+) ms, filter_record ([\d.]+) ms", text):
        out[f"{m.group(1)}: project_record (ms)"] = float(m.group(2))
        out[f"{m.group(1)}: filter_record (ms)"] = float(m.group(3))
    return out


def parse_pipeline(text):
    m = re.search(r"stages: scan ([\d.]+) ms, filter \+ project ([\d.]+) ms, write ([\d.]+) ms", text)
    d = re.search(r"^device \(.*?\): (\d+) ms", text, re.M)
    return {"device: filter + project stage (ms)": float(m.group(2)), "device: scan stage (ms)": float(m.group(1)),
            "device: write stage (ms)": float(m.group(3)), "device: end to end (ms)": float(d.group(1))}


def parse_bench(text):
    line = [ln for ln in text.splitlines() if ln.startswith("{")][-1]
    return {"headline (ms/step)": json.loads(line)["ms_per_step"]}


BENCHES = {   # name -> (command, seconds allowed, parser); every figure: lower is better
    "project_latency": ([sys.executable, "bench/micro/project_latency.py"], 240, parse_project_latency),
    "call_latency": ([sys.executable, "bench/micro/call_latency.py"], 240, parse_call_latency),
    "fused_probe": ([sys.executable, "bench/micro/fused_probe.py"], 300, parse_fused_probe),
    "nullable_projection": ([sys.executable, "bench/micro/nullable_projection.py"], 300, parse_nullable_projection),
    "pipeline": ([sys.executable, "bench/micro/pipeline.py"], 400, parse_pipeline),
    "bench": ([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5", "--no-cpu-baseline", "--no-extra"], 400, parse_bench),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--before", required=True, help="libchq.so of the build to compare against")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--only", action="append", choices=sorted(BENCHES), default=None)
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    result = {"runs_per_build": args.runs, "order": "before, after, before, after, ...", "lines": {}}
    for name in args.only or list(BENCHES):
        cmd, limit, parse = BENCHES[name]
        raw = {"before": {}, "after": {}}
        for _ in range(args.runs):
            for build in ("before", "after"):
                env = dict(os.environ)
                env.pop("CHQ_LIB_PATH", None)
                if build == "before":
                    env["CHQ_LIB_PATH"] = os.path.abspath(args.before)
                run = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=limit)
                if run.returncode != 0:   # nothing more is started after a failure
                    sys.exit(f"{name} ({build}) exited with {run.returncode}:\n{run.stdout[-2000:]}\n{run.stderr[-4000:]}")
                for key, value in parse(run.stdout).items():
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
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
