"""CPU tests of whole BAM files in (include/platypus_caller_bamfile.h) through the caller library linked against the CPU stand-in device:
plat_bam_file_open over files written in memory (tests/bam_file_cases.py) and its refusals; header text -> read groups and samples and
loadBAMData's decision against tests/golden/bam_header_cases.json.gz (the reference's own text, executed: README_bam_header.md);
plat_bam_files_fetch_plan under PLAT_CALLER_HOST_INDEX=1 against tabixindex's BAI rule and the cut by BSIZE; the refusal of
plat_call_bam_files without a device inflate; the structs against their ctypes mirrors; the Cython declarations; and the command line's
region list against getRegions' golden."""
import ctypes as C
import os
import struct
import subprocess
import sys

import pytest

from platypus_amd import _lib, fastcaller as F, synth
from platypus_amd.options import default_options
from tests import bam_file_cases as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return B.golden()


@pytest.fixture()
def nc(monkeypatch):
    from tests.fakedev import fake_caller_lib
    monkeypatch.setenv("PLAT_CALLER_HOST_INDEX", "1")
    c = F.NativeCaller(0, 1, 1, lib=fake_caller_lib())
    yield c
    c.close()


def _open(nc, f, **kw):
    b = f if "bam" in f else B.built(f, **kw)
    return nc.open_bam(b["bam"], b["bai"], b["name"]), b


def test_open_reads_names_lengths_read_groups_and_text_of_every_fixture(nc):
    for f in B.hand_files():
        for kw in (dict(), dict(header_payload=7), dict(header_payload=65280)):      # the header over ~50 blocks, and in one
            h, b = _open(nc, f, **kw)
            assert h.refs == [n.encode() for n, _ in f["refs"]] and h.lengths == [l for _, l in f["refs"]]
            assert [h.tid(n) for n, _ in f["refs"]] == list(range(len(f["refs"]))) and h.tid("chrZ") == -1 and h.tid(b"") == -1 and h.tid(b"chr\0A") == -1
            assert h.header_text == f["text"].encode()
            assert h.read_groups == f["groups"] and h.samples == f["samples"]
            assert (h.header_raised is None) == bool(f["groups"])
            assert h.header_sq == [(n.encode(), l) for n, l in f["refs"]]
            h.close()
    # a text cut at its first NUL byte, as Samfile.text cuts it; names are C strings too
    bam, bai, _ = B.write_bam(b"@RG\tID:a\tSM:s\n\0@RG\tID:b\tSM:t\n", [(b"c1\0junk", 100)], [])
    h = nc.open_bam(bam, bai, "z.bam")
    assert h.header_text == b"@RG\tID:a\tSM:s\n" and h.read_groups == [(b"a", b"s")] and h.refs == [b"c1"] and h.tid("c1") == 0
    h.close()
    assert nc.call_regions([], ["S1"], default_options()) == ""


def _bgzf(raw):
    return synth.bgzf_stream(raw, block_payload=50)[0]


def test_open_refuses_what_is_no_bam_file_and_the_caller_stays_usable(nc):
    good = B.built(B.two_contigs())
    head = B.bam_header(good["text"], good["refs"])
    l_text = len(good["text"])
    put = lambda at, v: head[:at] + struct.pack("<i", v) + head[at + 4:]
    name0 = 12 + l_text                                                     # l_name of the first reference
    cases = [
        ("no BGZF", b"this is not a BAM file at all, " * 4, "no BGZF stream"),
        ("an empty file", b"", "ends before"),
        ("only the EOF block", synth.BGZF_EOF, "ends before"),
        ("a bad magic", _bgzf(b"BAX\x01" + head[4:]), "bad magic"),
        ("a gzip file that is no BGZF", __import__("gzip").compress(head), "no BGZF stream"),
        ("l_text past the bytes", _bgzf(put(4, l_text + 100000)), "l_text runs past"),
        ("a negative l_text", _bgzf(put(4, -1)), "l_text is negative"),
        ("a negative n_ref", _bgzf(put(8 + l_text, -5)), "n_ref is negative"),
        ("n_ref past the bytes", _bgzf(put(8 + l_text, 3)), "n_ref runs past"),
        ("a negative l_name", _bgzf(put(name0, -2)), "l_name is negative"),
        ("l_name past the bytes", _bgzf(put(name0, 1 << 20)), "l_name runs past"),
        ("a header cut inside a block", good["bam"][:30], "no BGZF stream"),
        ("a corrupt block", good["bam"][:40] + bytes([good["bam"][40] ^ 0x55]) + good["bam"][41:], "no BGZF stream"),
    ]
    for why, data, words in cases:
        for _ in range(2):
            with pytest.raises(_lib.PlatypusDeviceError) as e:
                nc.open_bam(data, good["bai"], "x.bam")
            assert e.value.code == -9 and words in str(e.value), (why, str(e.value))
    one_ref = B.built(B.no_rg())
    for bai, words in ((one_ref["bai"], "holds 1 references, the file's header 2"), (b"not an index", ".bai"), (b"", ".bai")):
        with pytest.raises(_lib.PlatypusDeviceError) as e:
            nc.open_bam(good["bam"], bai, "x.bam")
        assert e.value.code == -9 and words in str(e.value)
    h = nc.open_bam(good["bam"], good["bai"], "x.bam")
    assert h.refs == [b"chrA", b"chrB"]
    h.close()
    assert nc.call_regions([], ["S1"], default_options()) == ""


def _header_file(text, name):
    bam, bai, _ = B.write_bam(text, [("chrA", 40000)], [])
    return dict(bam=bam, bai=bai, name=name)


def test_header_and_sample_rule_equal_the_reference_on_every_golden_header(nc, golden):
    assert len(golden["headers"]) >= 20
    labels = {h["label"] for h in golden["headers"]}
    assert {"no @RG", "an @RG without SM", "an unknown field code", "a line without @", "two @HD", "a duplicate ID", "SM containing ':'", "CRLF"} <= labels
    fell_back = 0
    for g in golden["headers"]:
        h, _ = _open(nc, _header_file(g["text"], g["file_name"]))
        assert sorted(h.samples) == [s.encode() for s in g["samples"]], g["label"]
        assert dict(h.read_groups) == {k.encode(): v.encode() for k, v in g["samplesByID"].items()}, g["label"]      # (a dict: the last of an ID wins)
        raised = isinstance(g["samplesByBAM"], str)                          # the reference's except branch leaves the NAME here, not a list
        assert (h.header_raised is not None) == raised, g["label"]
        if g["header_raised"] is not None:                                   # the getter itself raised: getRegions cannot read the @SQ lines either
            assert h.header_sq is None and h.read_groups == [], g["label"]
        elif g["header_rg"]:
            # header order, where every group has ID and SM
            if all(i is not None and s is not None for i, s in g["header_rg"]):
                assert h.read_groups == [(i.encode(), s.encode()) for i, s in g["header_rg"]], g["label"]
        fell_back += raised
        h.close()
    assert 8 <= fell_back < len(golden["headers"])


def test_plan_equals_loadBAMDatas_decision_on_every_golden_list_of_files(nc, golden):
    texts = {h["label"]: h["text"] for h in golden["headers"]}
    seen = set()
    for p in golden["plans"]:
        files = [_open(nc, _header_file(texts[f["label"]], f["file_name"]))[0] for f in p["files"]]
        seen.add(p["mode"])
        if p["mode"] == "assertion":
            for _ in range(2):
                with pytest.raises(_lib.PlatypusDeviceError) as e:
                    nc.bam_plan(files)
                assert e.value.code == -9 and "Something is screwy here" in str(e.value)
        else:
            got = nc.bam_plan(files)
            assert got["mode"] == p["mode"] and got["samples"] == [s.encode() for s in p["order"]], p["files"]
            assert got["samples"] == sorted(got["samples"])
            if p["mode"] == "presplit":
                assert got["sample_file"] == [p["chosen"][s] for s in p["order"]] and got["read_groups"] == []
            else:
                # the table is samplesByID with every SM as its place in the sample order; an ID whose SM is none of the call's samples is left out
                want = {k.encode(): p["order"].index(v) for k, v in p["samplesByID"].items() if v in p["order"]}
                assert got["sample_file"] is None and dict(got["read_groups"]) == want and len(got["read_groups"]) == len(want), p["files"]
        for f in files:
            f.close()
    assert seen == {"presplit", "merged", "assertion"}
    # the fixtures themselves
    built = {f["name"]: _open(nc, f)[0] for f in B.hand_files()}
    plan = nc.bam_plan([built["two_samples_merged.bam"]])
    assert plan == dict(mode="merged", samples=[b"T1", b"T2"], sample_file=None, read_groups=[(b"ga", 1), (b"gb", 0)])
    plan = nc.bam_plan([built["split_a.bam"], built["split_b.bam"]])
    assert plan == dict(mode="merged", samples=[b"ONE"], sample_file=None, read_groups=[(b"ra", 0), (b"rb", 0)])
    plan = nc.bam_plan([built["two_contigs.bam"], built["some/dir/no_rg.sample.bam"]])
    assert plan == dict(mode="presplit", samples=[b"NA1", b"no_rg.sample"], sample_file=[0, 1], read_groups=[])
    for h in built.values():
        h.close()


def test_fetch_plan_equals_the_bai_rule_and_the_cut_by_bsize(nc):
    a, b, one = B.built(B.two_contigs()), B.built(B.two_samples_merged()), B.built(B.no_rg())
    files = [nc.open_bam(f["bam"], f["bai"], f["name"]) for f in (a, b, one)]
    regions = [("chrA", 0, 5000), ("chrA", 1, 5000), ("chrA", 5000, 20000), ("chrB", 100, 29000), ("chrB", 28990, 29990), ("chrA", 39990, 40000),
               ("chrZ", 5, 50), ("chrA", 12345, 12346), ("chrA", 0, 1 << 29)]
    got = nc.bam_fetch_plan(files, regions)
    crossing = n_chunks = 0
    for (chrom, start, end), per in zip(regions, got):
        for f, g in zip((a, b, one), per):
            want = B.fetch(f, chrom, start, end)
            assert {k: g[k] for k in ("tid", "itr_beg", "itr_end")} == {k: want[k] for k in ("tid", "itr_beg", "itr_end")}, (chrom, start, end, f["name"])
            assert g["chunks"] == want["chunks"], (chrom, start, end, f["name"])
            n_chunks += len(g["chunks"])
            crossing += sum(1 for _, ln, _, ec, eu in g["chunks"] if ec > 0 and eu > 0)
    # start = 0 and start = 1 ask for the same window; a contig a file lacks leaves that file empty; chrB is not in the third file
    assert got[0][0]["itr_beg"] == got[1][0]["itr_beg"] == 0 and got[2][0]["itr_beg"] == 4999
    assert all(g["tid"] == -1 and g["chunks"] == [] for g in got[6]) and got[3][2]["tid"] == -1 and got[3][0]["tid"] == 1
    # fetches of several chunks, and chunks that end inside a later block than they begin in
    assert max(len(g[0]["chunks"]) for g in got) >= 2 and n_chunks >= 20 and crossing >= 5, (n_chunks, crossing)
    assert nc.bam_fetch_info["queries"] == nc.bam_fetch_info["handed_over"] == 3 * len(regions) - 3 - 2 and nc.bam_fetch_info["device_calls"] == 0
    # the kept records, by the rule, lie inside what was cut: every chunk list covers the virtual offsets of the records sam_itr_next keeps
    for (chrom, start, end), per in zip(regions[:6], got):
        want = B.fetch(a, chrom, start, end)
        kept = B.kept_records(a, chrom, start, end)
        los = [(c[0] << 16) | c[2] for c in want["chunks"]]
        his = [((c[0] + c[3]) << 16) | c[4] for c in want["chunks"]]
        for i in kept:
            u = a["placed"][i][3]
            assert any(lo <= u < hi for lo, hi in zip(los, his)), (chrom, start, end, i)
    # a window that is none: named
    for bad in (("chrA", 10, 9), ("chrA", 0, 0), ("chrB", 101, 100)):
        with pytest.raises(_lib.PlatypusDeviceError) as e:
            nc.bam_fetch_plan(files, [("chrA", 5, 50), bad])
        assert e.value.code == -1 and "region 1" in str(e.value) and "%s:%d-%d" % bad in str(e.value)
    assert nc.bam_fetch_plan(files, []) == []
    # a file cut short behind its header: a chunk whose block is not there is named, the offsets read off the file's own index
    from platypus_amd import tabixindex
    half = a["bam"][:len(a["bam"]) // 2]
    short = nc.open_bam(half, a["bai"], "short.bam")
    with pytest.raises(_lib.PlatypusDeviceError) as e:
        nc.bam_fetch_plan([short], [("chrA", 30000, 39000)])
    n, u, v = B.first_chunk_off_the_data(half, tabixindex.BamIndex(a["bai"]).query(0, *B.window(30000, 39000)))
    assert u >> 16 >= len(half) or v >> 16 >= len(half)
    entry = "plat_bam_files_fetch_plan"
    assert e.value.code == -9 and str(e.value) == str(_lib.PlatypusDeviceError(
        -9, "%s: chunk %d of region 0, file 0 (virtual offsets %d .. %d) %s" % (entry, n, u, v, B.NO_CUT), entry))
    short.close()
    for f in files:
        f.close()
    assert nc.call_regions([], ["S1"], default_options()) == ""


def test_fake_device_refuses_the_call_and_stays_usable(nc, monkeypatch):
    """The stand-in device has neither plat_index_query_batch nor plat_bgzf_inflate_batch: PLAT_ERR_UNSUPPORTED naming the symbol, twice,
    from both modes; and the pair of options that asks for broken mates is refused by name."""
    a, m = B.built(B.two_contigs()), B.built(B.two_samples_merged())
    for built, symbol in ((a, "plat_call_bgzf_regions: the device library has no plat_bgzf_inflate_batch"), (m, "plat_call_bgzf_regions_rg: the device library has no plat_bam_route_batch")):
        h = nc.open_bam(built["bam"], built["bai"], built["name"])
        region = F.BamFilesRegion("chrA", 100, 5000, b"ACGT" * 10000)
        for _ in range(2):
            with pytest.raises(_lib.PlatypusDeviceError) as e:
                nc.call_bam_files([h], [region], default_options())
            assert e.value.code == -6 and symbol in str(e.value)
        monkeypatch.delenv("PLAT_CALLER_HOST_INDEX")
        for _ in range(2):
            with pytest.raises(_lib.PlatypusDeviceError) as e:
                nc.call_bam_files([h], [region], default_options())
            assert e.value.code == -6 and "plat_index_query_batch" in str(e.value)
        monkeypatch.setenv("PLAT_CALLER_HOST_INDEX", "1")
        with pytest.raises(_lib.PlatypusDeviceError) as e:
            nc.call_bam_files([h], [region], default_options(assemble=1, assembleBrokenPairs=1))
        assert e.value.code == -6 and "assembleBrokenPairs" in str(e.value)
        h.close()
    assert nc.call_regions([], ["S1"], default_options()) == ""


def test_structs_match_their_ctypes_mirrors(tmp_path):
    F.build()
    src = tmp_path / "lay.c"
    src.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include "platypus_caller_bamfile.h"
int main(void){
  printf("%zu %zu %zu %zu %zu\n", sizeof(plat_bam_plan), offsetof(plat_bam_plan, n_samples), offsetof(plat_bam_plan, sample_names), offsetof(plat_bam_plan, sample_file),
         offsetof(plat_bam_plan, groups));
  printf("%zu %zu %zu %zu %zu\n", sizeof(plat_bam_call_region), offsetof(plat_bam_call_region, start), offsetof(plat_bam_call_region, contig_seq),
         offsetof(plat_bam_call_region, contig_len), offsetof(plat_bam_call_region, dev_contig_seq));
  printf("%zu %zu %zu %zu\n", sizeof(plat_bam_fetch), offsetof(plat_bam_fetch, itr_end), offsetof(plat_bam_fetch, n_chunks), offsetof(plat_bam_fetch, chunks));
  printf("%zu %zu %zu %zu %zu\n", sizeof(plat_bam_fetch_plan), offsetof(plat_bam_fetch_plan, n_files), offsetof(plat_bam_fetch_plan, fetches),
         offsetof(plat_bam_fetch_plan, queries), offsetof(plat_bam_fetch_plan, seconds));
  printf("%d %d\n", PLAT_BAM_FILES_PRESPLIT, PLAT_BAM_FILES_MERGED);
  { int (*fn)(plat_caller*, plat_bamfile* const*, int, const plat_bam_call_region*, int, plat_caller_options*, const plat_caller_qc_options*, char**, size_t*,
              plat_fetched_region_info*, plat_caller_stats*) = plat_call_bam_files;
    plat_bamfile* f = NULL; plat_bam_plan* p = NULL; plat_bam_fetch_plan* q = NULL;
    printf("%d %d %d %d %d\n", fn(NULL, NULL, 0, NULL, 0, NULL, NULL, NULL, NULL, NULL, NULL), plat_bam_file_open(NULL, NULL, 0, NULL, 0, "x", &f),
           plat_bam_files_plan(NULL, 0, &p), plat_bam_files_fetch_plan(NULL, 0, NULL, 0, &q), plat_bam_file_n_refs(NULL)); }
  return 0; }''')
    exe = tmp_path / "lay"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic-errors", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L" + os.path.dirname(F.LIB_PATH), "-lplat_caller", "-lplat_mi355x", "-Wl,-rpath," + os.path.dirname(F.LIB_PATH)])
    v = list(map(int, subprocess.check_output([str(exe)], text=True).split()))
    P, R, T, X = F._BamPlan, F._BamCallRegion, F._BamFetch, F._BamFetchPlan
    assert v[0:5] == [C.sizeof(P), P.n_samples.offset, P.sample_names.offset, P.sample_file.offset, P.groups.offset]
    assert v[5:10] == [C.sizeof(R), R.start.offset, R.contig_seq.offset, R.contig_len.offset, R.dev_contig_seq.offset]
    assert v[10:14] == [C.sizeof(T), T.itr_end.offset, T.n_chunks.offset, T.chunks.offset]
    assert v[14:19] == [C.sizeof(X), X.n_files.offset, X.fetches.offset, X.queries.offset, X.seconds.offset]
    assert v[19:21] == [F.BAM_FILES_MODES.index("presplit"), F.BAM_FILES_MODES.index("merged")]
    assert v[21:] == [-1, -1, -1, -1, -1]
    # the headers this one completes no longer say the opposite
    for name, gone in (("platypus_caller_index.h", "an entry point that takes whole BAM files"), ("platypus_caller_bgzf.h", "the BAM header, CRAM"),
                       ("platypus_caller_rg.h", "Not handled: parsing the @RG header lines")):
        with open(os.path.join(ROOT, "include", name)) as f:
            text = f.read()
        assert gone not in text and "platypus_caller_bamfile.h" in text, name


def test_cython_declarations_of_the_bam_file_entry_points_build(tmp_path):
    pytest.importorskip("Cython")
    pyx = tmp_path / "bamfile_check.pyx"
    pyx.write_text('''# cython: language_level=3
from libc.string cimport memset
cimport cplat

def sizes():
    cdef cplat.plat_bam_call_region r
    cdef cplat.plat_bamfile* f = NULL
    cdef cplat.plat_bam_plan* p = NULL
    cdef cplat.plat_bam_fetch_plan* q = NULL
    memset(&r, 0, sizeof(r))
    return (sizeof(cplat.plat_bam_plan), sizeof(cplat.plat_bam_fetch), sizeof(cplat.plat_bam_fetch_plan), sizeof(r),
            cplat.plat_bam_file_open(NULL, NULL, 0, NULL, 0, b"x", &f), cplat.plat_bam_files_plan(NULL, 0, &p),
            cplat.plat_bam_files_fetch_plan(NULL, 0, &r, 0, &q), cplat.plat_bam_file_n_refs(f), cplat.plat_bam_file_n_header_sq(f),
            cplat.plat_call_bam_files(NULL, NULL, 0, &r, 0, NULL, NULL, NULL, NULL, NULL, NULL))
''')
    c_file = tmp_path / "bamfile_check.c"
    subprocess.check_call([sys.executable, "-m", "cython", "-3", "-I", os.path.join(ROOT, "bindings"), str(pyx), "-o", str(c_file)])
    import sysconfig
    subprocess.check_call(["gcc", "-c", "-fPIC", "-O0", "-I" + sysconfig.get_paths()["include"], "-I" + os.path.join(ROOT, "include"), str(c_file),
                           "-o", str(tmp_path / "bamfile_check.o")])


def test_command_line_keeps_its_message_without_a_reference_file():
    r = subprocess.run([sys.executable, "-m", "platypus_amd", "callVariants", "--bamFiles", "x.bam"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode != 0
    assert ("platypus_amd: BAM/FASTA input needs the reference's htslib I/O layer, which is outside this build's scope (see DESIGN.md, 'out of scope').  "
            "Use --synthetic=config2[:N] or the in-memory API (platypus_amd.hostapi / include/platypus_mi355x.h).") in r.stderr
    r = subprocess.run([sys.executable, "-m", "platypus_amd", "callVariants", "--help"], capture_output=True, text=True, cwd=ROOT)
    assert "FILE.bai" in r.stdout and "platypus_caller_bamfile.h" in " ".join(r.stdout.split())


def test_command_line_region_list_equals_getRegions(nc, golden):
    from platypus_amd.__main__ import bam_regions
    texts = {h["label"]: h["text"] for h in golden["headers"]}
    assert len(golden["regions"]) >= 12
    from_fai = chunked = 0
    for g in golden["regions"]:
        h, _ = _open(nc, _header_file(texts[g["label"]], "x.bam"))
        sq = h.header_sq
        got = bam_regions(None if sq is None else [(n.decode(), l) for n, l in sq], [tuple(x) for x in g["fai"]], g["regions"], g["bufferSize"])
        assert [list(r) for r in got] == g["final"], (g["label"], g["regions"], g["bufferSize"])
        from_fai += sq is None
        chunked += len(g["final"]) > 2
        h.close()
    assert from_fai >= 2 and chunked >= 4
    with pytest.raises(ValueError):
        bam_regions([("chrA", 10)], [("chrA", 10)], ["chrA:5"], 100)           # (the reference's unpacking of split("-") raises too)
