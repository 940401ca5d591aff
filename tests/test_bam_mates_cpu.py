"""CPU tests of the broken-mate fetch (plat_bam_files_mates_plan, plat_call_bam_files_mates: include/platypus_caller_bamfile.h): the fixture
(tests/golden/broken_mate_cases.json.gz, README_broken_mates.md: the reference's own text, executed) pins csrc/mate_rule.hpp -- which
record gives a coordinate, the order of the coordinates, mergeQueries, the filter -- through tests/mate_rule_host_driver.cpp, a
stand-alone program that also runs under the sanitizers; the structs against their ctypes mirrors; and, through the stand-in device,
the refusals of the new call.  tests/test_gpu_bam_mates_kernel.py and tests/test_gpu_bam_mates.py run the device pass and the plan."""
import ctypes as C
import gzip
import json
import os
import subprocess

import pytest

from platypus_amd import _lib, fastcaller as F
from platypus_amd.options import default_options
from tests import bam_file_cases as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "broken_mate_cases.json.gz")


@pytest.fixture(scope="module")
def cases():
    with gzip.open(GOLDEN, "rt") as f:
        return json.load(f)["cases"]


def _driver_input(cases):
    out = []
    for c in cases:
        out.append("case %d %d %d %d %d %d" % (len(c["contigs"]), c["chrom_id"], c["start"], c["end"], len(c["reads"]), len(c["second"])))
        out.append(" ".join(c["contigs"]))
        out.extend("%d %d %d" % tuple(r) for r in c["reads"])
        out.extend("%d %d" % tuple(s) for s in c["second"])
    return "\n".join(out) + "\n"


def _driver_output(text):
    """Per case dict(picked, sorted, queries, windows, is_mate) from the driver's lines."""
    done, cur = [], dict(picked=[], sorted=[], queries=[], windows=[], is_mate=[])
    for line in text.split("\n")[:-1]:
        w = line.split(" ")
        if w[0] == "end":
            done.append(cur)
            cur = dict(picked=[], sorted=[], queries=[], windows=[], is_mate=[])
        elif w[0] == "Q":
            cur["queries"].append([w[1], int(w[2]), int(w[3])])
        else:
            cur[dict(P="picked", S="sorted", W="windows", M="is_mate")[w[0]]].append([int(x) for x in w[1:]] if w[0] != "M" else int(w[1]))
    return done


def _build_driver(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-g", "-std=c++17", "-Wall", "-Werror"] + flags + ["-I" + os.path.join(ROOT, "platypus_amd", "csrc"),
                           os.path.join(ROOT, "tests", "mate_rule_host_driver.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitizers"])
def test_rule_reproduces_every_golden_case(tmp_path, cases, flags):
    """Coordinates picked, their order, the queries and the filter's decisions of every case; the windows by the file's own rule."""
    exe = _build_driver(tmp_path, "mate_rule_driver", flags)
    path = tmp_path / "cases.txt"
    path.write_text(_driver_input(cases))
    got = _driver_output(subprocess.check_output([exe, str(path)], text=True))
    assert len(got) == len(cases) >= 28
    for c, g in zip(cases, got):
        assert g["picked"] == c["picked"], c["label"]
        assert g["sorted"] == c["sorted"], c["label"]
        assert g["queries"] == c["queries"], c["label"]
        assert g["is_mate"] == c["is_mate"], c["label"]
        assert g["windows"] == [[max(s - 1, 0), min(e, 2 ** 31 - 1)] for _, s, e in c["queries"]], c["label"]


def test_the_golden_holds_the_cases_it_was_asked_for(cases):
    by = {c["label"]: c for c in cases}
    assert by["the empty list"]["picked"] == [] and by["the empty list"]["queries"] == []
    assert len(by["one coordinate"]["queries"]) == 1 and len(by["equal coordinates"]["picked"]) == 3 and len(by["equal coordinates"]["queries"]) == 1
    assert [len(by["a gap of %d" % g]["queries"]) for g in (9999, 10000, 10001)] == [1, 2, 2]
    assert [len(by["a span of %d" % s]["queries"]) for s in (99999, 100000, 100001)] == [1, 2, 2]
    c = by["two contigs, name order against tid order"]
    assert c["contigs"] == ["chrB", "chrA"] and [q[0] for q in c["queries"]] == sorted(q[0] for q in c["queries"]) and c["queries"][0][0] == "chrA"
    assert by["mtid -1 under every flag"]["picked"] == []
    for label in ("every flag, mate on the same contig", "every flag, mate on the other contig"):
        flags = [r[0] & 14 for r in by[label]["reads"]]
        assert sorted(flags) == [0, 2, 4, 6, 8, 10, 12, 14] and len(by[label]["picked"]) == 7     # (only 0x2 alone is a proper, mapped pair)
    c = by["one coordinate"]
    want = {(c["chrom_id"], c["start"] - 1): 0, (c["chrom_id"], c["start"]): 1, (c["chrom_id"], c["end"]): 1, (c["chrom_id"], c["end"] + 1): 0}
    for (t, p), m in zip(c["second"], c["is_mate"]):
        if (t, p) in want:
            assert m == want.pop((t, p))
    assert not want


def test_structs_match_their_ctypes_mirrors(tmp_path):
    F.build()
    src = tmp_path / "lay.c"
    src.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include "platypus_mi355x.h"
#include "platypus_caller_bamfile.h"
int main(void){
  printf("%zu %zu %zu %zu\n", sizeof(plat_bam_mate_query), offsetof(plat_bam_mate_query, tid), offsetof(plat_bam_mate_query, start), offsetof(plat_bam_mate_query, end));
  printf("%zu %zu %zu %zu %zu\n", sizeof(plat_bam_mates), offsetof(plat_bam_mates, n_coords), offsetof(plat_bam_mates, n_queries), offsetof(plat_bam_mates, queries),
         offsetof(plat_bam_mates, mates));
  printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(plat_bam_mates_plan), offsetof(plat_bam_mates_plan, n_files), offsetof(plat_bam_mates_plan, units),
         offsetof(plat_bam_mates_plan, loaded), offsetof(plat_bam_mates_plan, coords), offsetof(plat_bam_mates_plan, records_kept), offsetof(plat_bam_mates_plan, input_bytes),
         offsetof(plat_bam_mates_plan, seconds));
  printf("%zu %zu %zu %zu %zu %zu\n", sizeof(plat_bam_mates_in), offsetof(plat_bam_mates_in, mode), offsetof(plat_bam_mates_in, data), offsetof(plat_bam_mates_in, data_len),
         offsetof(plat_bam_mates_in, stream_begin), offsetof(plat_bam_mates_in, hi));
  printf("%zu %zu %zu %zu %zu %zu\n", sizeof(plat_bam_mates_out), offsetof(plat_bam_mates_out, cap_bytes), offsetof(plat_bam_mates_out, coords),
         offsetof(plat_bam_mates_out, out_data), offsetof(plat_bam_mates_out, status), offsetof(plat_bam_mates_out, need_bytes));
  printf("%d %d\n", PLAT_MATES_COORDS, PLAT_MATES_FETCH);
  { int (*fn)(plat_caller*, plat_bamfile* const*, int, const plat_bam_call_region*, int, plat_caller_options*, const plat_caller_qc_options*, char**, size_t*,
              plat_fetched_region_info*, plat_caller_stats*) = plat_call_bam_files_mates;
    plat_bam_mates_plan* p = NULL;
    printf("%d %d\n", fn(NULL, NULL, 0, NULL, 0, NULL, NULL, NULL, NULL, NULL, NULL), plat_bam_files_mates_plan(NULL, 0, NULL, 0, NULL, NULL, &p));
    plat_bam_mates_plan_free(p); }
  return 0; }''')
    exe = tmp_path / "lay"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic-errors", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L" + os.path.dirname(F.LIB_PATH), "-lplat_caller", "-lplat_mi355x", "-Wl,-rpath," + os.path.dirname(F.LIB_PATH)])
    v = list(map(int, subprocess.check_output([str(exe)], text=True).split()))
    Q, M, P, I, O = F._BamMateQuery, F._BamMates, F._BamMatesPlan, _lib.BamMatesIn, _lib.BamMatesOut
    assert v[0:4] == [C.sizeof(Q), Q.tid.offset, Q.start.offset, Q.end.offset]
    assert v[4:9] == [C.sizeof(M), M.n_coords.offset, M.n_queries.offset, M.queries.offset, M.mates.offset]
    assert v[9:17] == [C.sizeof(P), P.n_files.offset, P.units.offset, P.loaded.offset, P.coords.offset, P.records_kept.offset, P.input_bytes.offset, P.seconds.offset]
    assert v[17:23] == [C.sizeof(I), I.mode.offset, I.data.offset, I.data_len.offset, I.stream_begin.offset, I.hi.offset]
    assert v[23:29] == [C.sizeof(O), O.cap_bytes.offset, O.coords.offset, O.out_data.offset, O.status.offset, O.need_bytes.offset]
    assert v[29:31] == [_lib.MATES_COORDS, _lib.MATES_FETCH]
    assert v[31:] == [-1, -1]
    # the documents no longer say the fetch is missing
    with open(os.path.join(ROOT, "include", "platypus_caller_bamfile.h")) as f:
        text = f.read()
    assert "are not fetched" not in text and "plat_call_bam_files_mates" in text
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        assert "Broken mates: not built" not in f.read()


@pytest.fixture()
def nc(monkeypatch):
    from tests.fakedev import fake_caller_lib
    monkeypatch.setenv("PLAT_CALLER_HOST_INDEX", "1")
    c = F.NativeCaller(0, 1, 1, lib=fake_caller_lib())
    yield c
    c.close()


def test_fake_device_refuses_the_mates_call_by_symbol_and_stays_usable(nc):
    """The stand-in device has no plat_bam_mates_batch: with both options set the call and the plan return PLAT_ERR_UNSUPPORTED naming it,
    twice, from both modes; with either option 0 the call refuses exactly as call_bam_files does."""
    a, m = B.built(B.two_contigs()), B.built(B.two_samples_merged())
    both = dict(assemble=1, assembleBrokenPairs=1)
    for built in (a, m):
        h = nc.open_bam(built["bam"], built["bai"], built["name"])
        region = F.BamFilesRegion("chrA", 100, 5000, b"ACGT" * 10000)
        for _ in range(2):
            with pytest.raises(_lib.PlatypusDeviceError) as e:
                nc.call_bam_files_mates([h], [region], default_options(**both))
            assert e.value.code == -6 and "the device library has no plat_bam_mates_batch" in str(e.value) and "plat_call_bam_files_mates" in str(e.value)
        for _ in range(2):
            with pytest.raises(_lib.PlatypusDeviceError) as e:
                nc.bam_mates_plan([h], [("chrA", 100, 5000)], default_options(**both))
            assert e.value.code == -6 and "plat_bam_files_mates_plan: the device library has no plat_bam_mates_batch" in str(e.value)
        for off in (dict(), dict(assemble=1), dict(assembleBrokenPairs=1)):
            said = []
            for call in (nc.call_bam_files, nc.call_bam_files_mates):
                with pytest.raises(_lib.PlatypusDeviceError) as e:
                    call([h], [region], default_options(**off))
                said.append((e.value.code, str(e.value).replace("plat_call_bam_files_mates", "plat_call_bam_files")))
            assert said[0] == said[1] and said[0][0] == -6 and "the device library has no" in said[0][1]
        # plat_call_bam_files itself still refuses the pair of options, and says where to go
        with pytest.raises(_lib.PlatypusDeviceError) as e:
            nc.call_bam_files([h], [region], default_options(**both))
        assert e.value.code == -6 and "assembleBrokenPairs" in str(e.value) and "plat_call_bam_files_mates" in str(e.value)
        h.close()
    assert nc.call_regions([], ["S1"], default_options()) == ""
