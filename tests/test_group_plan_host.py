"""CPU tier of the batch-group filter: its planning unit (csrc/group_plan.cpp: eligibility, tiling, the layout and the writer of
the group table, the fold's size rule, chunk cuts, the concat tables) without a GPU.  tests/group_plan_main.cpp plans every
case described here under the host sanitizers, checks the plans against the invariants the kernels rely on and writes them
out as text; here every plan is compared with the independent model of tests/group_plan_reference.py."""
import itertools
import os
import re
import shutil
import subprocess

import pytest

from tests import group_plan_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK_BYTES = 1 << 20                    # low enough that the 64-batch group is cut and its strings do not fit one column
BYTES_PER_ROW = (8, 24, 40)              # of the Utf8 columns, in order (the program's kBytesPerRow): the third is a long string
CHECKS_PER_CASE = 16
PUT_COLUMN_CHECKS = 15                   # put_column on real host bitmaps: counted over the slice, all-set is no bitmap, offsets applied

GROUPS = {"two_by_two": (0, [2, 2])}
for n in (1023, 1024, 1025, 2047, 2048, 2049, 16383, 16384, 16385):
    GROUPS["uniform_%d" % n] = (0, [n] * 3)
for n in (16383, 16384, 16385):          # one outlier among 10 000-row batches
    GROUPS["outlier_%d" % n] = (0, [10000] * 4 + [n] + [10000] * 3)
GROUPS["reference_64"] = (0, [10000] * 64)
GROUPS["ragged"] = (0, [2, 16385, 513])
# the w * nb < 2^31 - 64 edge of wave packing, by counts alone: two batches of (2^30 - 32) resp. (2^30 - 33) waves of the large tile
GROUPS["edge_at"] = (1, [(2**30 - 32) * 1024] * 2)
GROUPS["edge_below"] = (1, [(2**30 - 33) * 1024] * 2)

DIMS = {"tile_kind": [-1, 0, 1, 2], "mode": [0, 1, 2], "fixed": [1, 3, R.MAX_OUT], "utf8": [0, 1, 2, 3], "bool": [0, 1], "nulls": [0, 1, 17],
        "refs": list(range(R.MAX_REFS + 1))}
ORDER = ["tile_kind", "mode", "fixed", "utf8", "bool", "nulls", "refs"]
# beyond the cross: wide predicates, host and mixed residency, the options off, the flaws that send a group to the per-batch loop
EXTRA = [(g, tk, mode, fixed, utf8, bo, nulls, 2, wide, resid, gb, fu, gf, flaw)
         for g in ("uniform_1025", "reference_64", "ragged") for tk, mode in ((-1, 0), (1, 2))
         for fixed, utf8, bo, nulls, wide, resid, gb, fu, gf, flaw in (
             (3, 0, 0, 0, 1, "device", 1, 1, 1, "none"), (3, 1, 0, 0, 1, "device", 1, 1, 1, "none"), (3, 0, 0, 0, 0, "host", 1, 1, 1, "none"),
             (3, 0, 1, 1, 0, "host", 1, 1, 1, "none"), (3, 1, 0, 0, 0, "host", 1, 1, 1, "none"), (3, 0, 0, 0, 0, "mixed", 1, 1, 1, "none"),
             (3, 0, 1, 1, 0, "device", 0, 1, 1, "none"), (3, 1, 0, 1, 0, "device", 0, 1, 1, "none"), (3, 1, 0, 0, 0, "device", 1, 0, 1, "none"),
             (3, 2, 0, 0, 0, "device", 1, 1, 0, "none"), (3, 0, 0, 0, 0, "device", 1, 1, 1, "short"), (3, 1, 1, 1, 0, "device", 1, 1, 1, "schema"),
             (3, 2, 0, 0, 0, "device", 1, 1, 1, "nodata"))]


def schema_of(fixed, utf8, boolean):
    """the program's schema_of: fixed column 0, the Utf8 columns, the other fixed columns, the Boolean column"""
    return "f" + "u" * utf8 + "f" * (fixed - 1) + "b" * boolean


@pytest.fixture(scope="module")
def planned(tmp_path_factory):
    """the plan lines of every case, after the program's own checks passed under the sanitizers"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler on PATH")
    out = tmp_path_factory.mktemp("group_plan")
    exe = str(out / "group_plan_main")
    flags = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    src = os.path.join(ROOT, "tests", "group_plan_main.cpp")
    build = subprocess.run([cxx, *flags, "-static-libasan", "-static-libubsan", src, "-o", exe], capture_output=True, text=True)
    if build.returncode != 0:
        build = subprocess.run([cxx, *flags, src, "-o", exe], capture_output=True, text=True)
    if build.returncode != 0 and re.search(r"asan|ubsan|sanitize", build.stderr, re.I):
        pytest.skip("the compiler has no sanitizer runtime: " + build.stderr.strip().splitlines()[-1])
    assert build.returncode == 0, build.stderr
    with open(out / "groups.txt", "w") as f:
        f.write("chunk %d\n" % CHUNK_BYTES)
        for name in ORDER:
            f.write("dim %s %s\n" % (name, " ".join(map(str, DIMS[name]))))
        for name, (big, rows) in GROUPS.items():
            f.write("group %s %d %s\n" % (name, big, " ".join(map(str, rows))))
        for name in GROUPS:
            f.write("cross %s\n" % name)
        for case in EXTRA:
            f.write("case " + " ".join(map(str, case)) + "\n")
    run = subprocess.run([exe, str(out / "groups.txt"), str(out / "plans.txt")], capture_output=True, text=True)
    if run.returncode != 0 and "runtime does not come first" in run.stderr:
        pytest.skip("this environment preloads a library in front of the sanitizer runtime: " + run.stderr.strip().splitlines()[0])
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    cases = len(GROUPS) * len(list(itertools.product(*DIMS.values()))) + len(EXTRA)
    m = re.fullmatch(r"(\d+) checks, 0 mismatches\n", run.stdout)
    assert m and int(m.group(1)) == CHECKS_PER_CASE * cases + PUT_COLUMN_CHECKS, (run.stdout, cases)      # 16 invariants on each of the 191 022 cases
    with open(out / "plans.txt") as f:
        lines = f.read().splitlines()
    assert len(lines) == cases
    return lines


def expected(group, tile_kind, mode, fixed, utf8, boolean, nulls, refs, wide, residency, group_bits, fold_utf8, group_fold, flaw):
    """the sections of one plan line, from the model"""
    rows = list(GROUPS[group][1])
    if flaw == "short":
        rows[-1] = 1
    rows = tuple(rows)
    nb, total = len(rows), sum(rows)
    schema = schema_of(fixed, utf8, boolean)
    n_null = min(nulls, len(schema))
    e = R.eligibility(schema, flaw == "short", flaw == "schema", residency == "host", residency == "device", n_null > 0, flaw == "nodata" and utf8 > 0,
                      {"group_bits": group_bits, "fold_utf8": fold_utf8, "group_fold": group_fold, "host_in": residency == "host", "total_rows": total})
    if e["per_batch"]:      # nothing else is decided
        e = {"per_batch": True, "plain": False, "fold": False, "need_bits": False, "resident": False, "n_fold": 0}
        plan = [1, 0, 0, 0, 0, 0, 0, 0]
    else:
        plan = [0, int(e["plain"]), int(e["fold"]), int(e["need_bits"]), int(e["resident"]), total, max(rows), e["n_fold"]]
    kind, wpb, ntiles = R.tiling(rows, bool(wide), tile_kind, mode)
    n_bits = boolean + n_null if e["need_bits"] else 0
    lay = R.table_layout(kind, wpb, ntiles, nb, refs, fixed, e["n_fold"], e["need_bits"], n_bits)
    n_sized = e["n_fold"] if e["fold"] else utf8
    caps = [total * BYTES_PER_ROW[u] for u in range(n_sized)]
    fits, short = R.fold_verdict(caps, total, CHUNK_BYTES)
    c = R.cuts(rows, tuple(tuple(r * BYTES_PER_ROW[u] for r in rows) for u in range(n_sized)), CHUNK_BYTES)
    return {"plan": plan, "tiling": [kind, wpb, ntiles], "layout": [0] * 7 if lay is None else [1, *lay], "sizes": [int(fits), int(short), *caps],
            "cuts": [int(R.sub_groups(c)), *c], "concat": [R.concat_words(schema, nb, set(range(n_null)))]}


def test_every_plan_equals_the_model(planned):
    """eligibility, tile kind / waves per batch / tiles, stride and bits_at and the byte sizes of the table, the declines, the
    fold verdict and capacities, the cuts and the sub-group rule, the words of the concat tables: equal for every case"""
    seen = set()
    facts = {"packed": 0, "per_tile": 0, "declined": 0, "fold": 0, "bits": 0, "cut": 0, "per_batch": 0}
    for line in planned:
        head, *sections = line.split(" | ")
        w = head.split(" ")
        assert w[0] == "case"
        params = (w[1], *map(int, w[2:10]), w[10], *map(int, w[11:14]), w[14])
        assert params not in seen, line
        seen.add(params)
        want = expected(*params)
        got = {s.split(" ")[0]: [int(v) for v in s.split(" ")[1:]] for s in sections}
        assert got == want, (line, want)
        facts["packed"] += got["tiling"][1] > 0
        facts["per_tile"] += got["tiling"][1] == 0
        facts["declined"] += got["layout"][0] == 0
        facts["fold"] += got["plan"][2]
        facts["bits"] += got["layout"][2] > 0
        facts["cut"] += len(got["cuts"]) > 3
        facts["per_batch"] += got["plan"][0]
    cross = {(g, *v, 0, "device", 1, 1, 1, "none") for g in GROUPS for v in itertools.product(*(DIMS[n] for n in ORDER))}
    assert seen == cross | set(EXTRA)
    assert all(facts.values()), facts      # every kind of verdict did occur


def test_the_edges_fall_where_the_rules_put_them(planned):
    """single plans read off the rules by hand"""
    def tiling(group, tile_kind, mode):
        line = next(ln for ln in planned if ln.startswith("case %s %d %d 1 0 0 0 0 0 device" % (group, tile_kind, mode)))
        return [int(v) for v in line.split(" | ")[2].split(" ")[1:]]
    assert tiling("edge_below", -1, 0) == [0, 2**30 - 33, (2 * (2**30 - 33) + 15) // 16]     # 2^31 - 66 waves: packed
    assert tiling("edge_at", -1, 0) == [0, 0, 2 * (2**30 - 32) // 16]                          # 2^31 - 64 waves: per-tile table, large tiles
    assert tiling("uniform_1024", -1, 0) == [0, 1, 1] and tiling("uniform_1025", -1, 0) == [1, 0, 3]   # 2 waves for 1025 rows idle 37 %
    assert tiling("uniform_1025", 1, 0) == [1, 0, 3] and tiling("uniform_1024", 1, 0) == [1, 2, 2]     # small tile: 3 waves of 512 idle 33 %; 2 waves none
    assert tiling("reference_64", -1, 0) == [0, 10, 40] and tiling("reference_64", -1, 1) == [1, 0, 320]
    assert tiling("ragged", -1, 0) == [1, 0, 1 + 9 + 1] and tiling("ragged", -1, 2) == [0, 17, 4]
