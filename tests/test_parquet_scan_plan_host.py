"""CPU tier of the Parquet scan: its planning unit (csrc/parquet_scan_plan.cpp: column classification, the page loop of a
chunk, inflate jobs, wave cuts, launch chains) without a GPU.  tests/parquet_scan_plan_main.cpp plans every column of every
row group of the files of tests/parquet_plan_files.py under the host sanitizers, checks the plans against the invariants the
kernels rely on and writes them out as text; here the plans are compared with what an independent reader of the page headers
(tests/snappy_forge.py) and pyarrow's metadata say about the same bytes, the values of uncompressed PLAIN pages are cut out
of the file at the planned offsets and compared with pyarrow's, and every refusal is compared with the code and message the
GPU tier expects of the scan."""
import io
import os
import re
import shutil
import subprocess

import numpy as np
import pyarrow.parquet as pq
import pytest

from tests import parquet_plan_files as PF
from tests import snappy_forge as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMAT = {"BOOLEAN": ("b", 1), "INT32": ("i", 4), "INT64": ("l", 8), "FLOAT": ("f", 4), "DOUBLE": ("g", 8), "BYTE_ARRAY": ("u", 0)}
LIST = {0: "plain", 2: "dict", 8: "dict", 3: "rle"}            # Encoding of a data page -> the page list that serves it
DTYPE = {"i": "<i4", "l": "<i8", "f": "<f4", "g": "<f8"}


def parse_plan(text: str):
    """[row group] -> {"rows", "cols": [{"name", "error" | "class", "dict", "pages", "jobs"}]}"""
    groups = []
    for line in text.splitlines():
        w = line.split(" ")
        if w[0] == "rg":
            groups.append({"rows": int(w[3]), "cols": []})
        elif w[0] == "col":
            groups[-1]["cols"].append({"name": line.split(" ", 2)[2], "pages": [], "jobs": []})
        elif w[0] == "error":
            groups[-1]["cols"][-1]["error"] = (int(w[1]), line.split(" ", 2)[2])
        elif w[0] == "class":
            groups[-1]["cols"][-1]["class"] = {k: (v if k == "format" else int(v)) for k, v in zip(w[1::2], w[2::2])}
        elif w[0] == "dict":
            groups[-1]["cols"][-1]["dict"] = {k: int(v) for k, v in zip(w[1::2], w[2::2])}
        elif w[0] == "page":
            groups[-1]["cols"][-1]["pages"].append({"rows": int(w[3]), "first_row": int(w[5]), "levels": (int(w[7]), int(w[8])),
                                                    "values": (int(w[10]), int(w[11])), "list": w[13]})
        elif w[0] == "job":
            groups[-1]["cols"][-1]["jobs"].append({"src": (int(w[2]), int(w[3])), "dst": (int(w[5]), int(w[6])), "codec": int(w[8]),
                                                   "page": int(w[10]), "flags": int(w[12])})
        else:
            raise AssertionError(line)
    return groups


@pytest.fixture(scope="module")
def planned(tmp_path_factory):
    """name -> (bytes, plan text) of every file, after the program's own checks passed under the sanitizers"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler on PATH")
    out = tmp_path_factory.mktemp("parquet_scan_plan")
    exe = str(out / "parquet_scan_plan_main")
    flags = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    src = os.path.join(ROOT, "tests", "parquet_scan_plan_main.cpp")
    build = subprocess.run([cxx, *flags, "-static-libasan", "-static-libubsan", src, "-o", exe], capture_output=True, text=True)
    if build.returncode != 0:
        build = subprocess.run([cxx, *flags, src, "-o", exe], capture_output=True, text=True)
    if build.returncode != 0 and re.search(r"asan|ubsan|sanitize", build.stderr, re.I):
        pytest.skip("the compiler has no sanitizer runtime: " + build.stderr.strip().splitlines()[-1])
    assert build.returncode == 0, build.stderr
    files = {**PF.pyarrow_files(), **PF.forged_files(), **{n: v[0] for n, v in PF.host_refused().items()}}
    stems = {name: "f%04d" % k for k, name in enumerate(files)}
    for name, raw in files.items():
        with open(out / (stems[name] + ".parquet"), "wb") as f:
            f.write(raw)
    with open(out / "files.txt", "w") as f:
        f.write("".join(s + "\n" for s in stems.values()))
    run = subprocess.run([exe, str(out)], capture_output=True, text=True)
    if run.returncode != 0 and "runtime does not come first" in run.stderr:
        pytest.skip("this environment preloads a library in front of the sanitizer runtime: " + run.stderr.strip().splitlines()[0])
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    m = re.fullmatch(r"(\d+) checks, 0 mismatches\n", run.stdout)
    # 9 invariants per planned column chunk (1460 chunks) + 1156 on synthetic chains + 99 on wave cuts and parts
    assert m and int(m.group(1)) == 14395, run.stdout
    plans = {}
    for name, raw in files.items():
        with open(out / (stems[name] + ".plan")) as f:
            plans[name] = (raw, f.read())
    return plans


def check_against_the_headers(name: str, raw: bytes, groups, values: bool):
    """the plan of one file against the page headers as tests/snappy_forge.py reads them and pyarrow's footer; `values`: cut
    the uncompressed PLAIN fixed-width pages of required columns out of the file and compare with pyarrow's decode"""
    pf = pq.ParquetFile(io.BytesIO(raw))
    md = pf.metadata
    assert len(groups) == md.num_row_groups, name
    headers = {}
    for info, _payload in S.pages(raw):
        headers.setdefault((info.row_group, info.column), []).append(info)
    for g, got in enumerate(groups):
        rg = md.row_group(g)
        assert got["rows"] == rg.num_rows and len(got["cols"]) == rg.num_columns, (name, g)
        table = pf.read_row_group(g) if values else None
        for ci, col in enumerate(got["cols"]):
            where = (name, g, ci)
            assert "error" not in col, (where, col.get("error"))
            cm, k = rg.column(ci), col["class"]
            sc = md.schema.column(ci)
            assert col["name"] == sc.name and (k["format"], k["width"]) == FORMAT[cm.physical_type], where
            assert k["optional"] == (sc.max_definition_level == 1) and k["compressed"] == (cm.compression == "SNAPPY"), where
            assert (k["byte_array"], k["boolean"]) == (cm.physical_type == "BYTE_ARRAY", cm.physical_type == "BOOLEAN"), where
            st = cm.statistics
            assert k["has_levels"] == (k["optional"] and not (st is not None and st.has_null_count and st.null_count == 0)), where
            if rg.num_rows:
                first = cm.dictionary_page_offset if cm.has_dictionary_page else cm.data_page_offset
                assert (k["first"], k["csize"]) == (first, cm.total_compressed_size), where
            else:
                assert (k["first"], k["csize"]) == (0, 0) and not col["pages"] and not col["jobs"], where
                continue
            hs = headers[(g, ci)]
            data = [h for h in hs if h.type in (S.DATA_PAGE, S.DATA_PAGE_V2)]
            dic = [h for h in hs if h.type == S.DICTIONARY_PAGE]
            assert len(data) + len(dic) == len(hs) and len(col["pages"]) == len(data), where
            sub = [h.header.get(5) if h.type == S.DATA_PAGE else h.header.get(8) for h in data]
            assert [p["rows"] for p in col["pages"]] == [s.get(1) for s in sub], where                     # rows per page
            assert [p["list"] for p in col["pages"]] == [LIST[s.get(2) if h.type == S.DATA_PAGE else s.get(4)] for h, s in zip(data, sub)], where
            assert [p["first_row"] for p in col["pages"]] == list(np.cumsum([0] + [p["rows"] for p in col["pages"]])[:-1]), where
            assert sum(p["rows"] for p in col["pages"]) == rg.num_rows, where
            if dic:
                assert col["dict"]["count"] == dic[0].header.get(7).get(1) and col["dict"]["len"] == dic[0].header.get(2), where
            assert col["dict"]["walked"] == (k["byte_array"] and not k["compressed"] and any(p["list"] == "dict" for p in col["pages"])), where
            if k["compressed"]:      # one or two jobs a page; together they read every payload byte of the chunk once
                assert sum(j["src"][1] for j in col["jobs"]) == sum(h.header.get(3) for h in hs), where
                assert sum(j["dst"][1] for j in col["jobs"]) == sum(h.header.get(2) for h in hs), where
            if values and not k["compressed"] and not k["optional"] and k["format"] in DTYPE:
                want = table.column(ci).to_numpy()
                for p in col["pages"]:
                    if p["list"] != "plain":
                        continue
                    at = first + p["values"][0]
                    cut = np.frombuffer(raw[at:at + p["values"][1]], dtype=DTYPE[k["format"]])
                    assert p["values"][1] == p["rows"] * k["width"], where
                    assert np.array_equal(cut.view(np.uint8), want[p["first_row"]:p["first_row"] + p["rows"]].view(np.uint8)), (where, p)


def test_pyarrow_written_files_are_planned_as_their_headers_say(planned):
    """required and optional columns of all six physical types, V1 and V2 pages, PLAIN and dictionary encodings (and the
    writer's fall-back from one to the other), several pages a chunk, an empty row group, with and without statistics,
    uncompressed and snappy"""
    names = list(PF.pyarrow_files())
    assert len(names) == 20
    cut = 0
    for name in names:
        raw, text = planned[name]
        groups = parse_plan(text)
        check_against_the_headers(name, raw, groups, values=True)
        cut += sum(1 for g in groups for c in g["cols"] for p in c["pages"]
                   if p["list"] == "plain" and not c["class"]["compressed"] and not c["class"]["optional"] and c["class"]["format"] in DTYPE)
    # the value comparison did run: four uncompressed PLAIN files x four required fixed-width columns x two row groups, a page or more each
    assert cut >= 4 * 4 * 2
    multi = parse_plan(planned["six_none_v1_plain_2000"][1])
    assert all(len(c["pages"]) >= 3 for c in multi[0]["cols"] if c["class"]["format"] != "b")          # (several pages a chunk)
    assert [g["rows"] for g in parse_plan(planned["empty_row_group_snappy"][1])] == [400, 0, 300]


def test_forged_files_are_planned_as_their_headers_say(planned):
    """every case of the two forged suites; the damaged ones too: their defects lie in the value, level and snappy streams,
    which only the device reads (its "... of column ... are malformed") -- the host plans them like any file"""
    names = [n for n in planned if n.startswith(("forged ", "snappy "))]
    assert len(names) == 439 and set(PF.DEVICE_DAMAGE) <= set(names)
    for name in names:
        raw, text = planned[name]
        check_against_the_headers(name, raw, parse_plan(text), values=False)


def test_what_the_host_refuses_has_the_code_and_message_of_the_scan(planned):
    """the refusals the GPU tier expects of read_row_group (tests/test_gpu_parquet.py: unsupported codecs, a logical type, an
    encoding; an oversized level section) come from the planning unit, with the same code and text; a column in front of the
    defect is planned"""
    for name, (_raw, code, message) in PF.host_refused().items():
        groups = parse_plan(planned[name][1])
        errors = [(g, ci, c["error"]) for g, rg in enumerate(groups) for ci, c in enumerate(rg["cols"]) if "error" in c]
        assert errors and errors[0][2] == (code, message), (name, errors)
        if name.startswith("levels_past_page"):
            assert [(g, ci) for g, ci, _ in errors] == [(1, 0)] and len(groups[0]["cols"][0]["pages"]) == 1 and len(groups[1]["cols"][1]["pages"]) == 1
