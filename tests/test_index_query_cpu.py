"""CPU tests of the index query (plat_index_query_batch, include/platypus_caller_index.h): the fixture pins the rule's Python statement
(platypus_amd.tabixindex.TabixIndex.query) to the chunk lists the reference's ti_iter_query returned; the HOST TWIN (csrc/index_query.hpp:
built alone under AddressSanitizer and UBSan where libasan is installed) flattens every index to the tables the mirror makes and answers
every query as the mirror does, on the fixture, the older goldens and the hand-made indexes, as .tbi and as .bai; every prefix of a small
index is refused and never read past; the data-parallel restatement of the reference's three loops equals them on seeded random lists.
Through the stand-in device: the caller library refuses cleanly without plat_index_query_batch, and with PLAT_CALLER_HOST_INDEX=1 takes
whole files and returns the golden lines, byte for byte what plat_caller_set_source_blocks sets."""
import ctypes as C
import gzip
import os
import struct
import subprocess

import pytest

from platypus_amd import _lib, fastcaller as F, tabixindex
from platypus_amd.options import default_options
from tests import index_query_cases as Q, tabix_cases as T
from tests.bam_file_cases import NO_CUT, first_chunk_off_the_data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TBI, BAI = 0, 1


def all_indexes():
    """[(label, kind, raw bytes as the flatten takes them, index object, queries, prefixes)]"""
    out = []
    for f in Q.golden_files():
        out.append(("fixture " + f["label"], TBI, gzip.decompress(f["tbi"]), tabixindex.TabixIndex(f["tbi"]), [(q["tid"], q["beg"], q["end"]) for q in f["queries"]], False))
    for f in T.golden_files():
        out.append(("golden " + f["label"], TBI, gzip.decompress(f["tbi"]), tabixindex.TabixIndex(f["tbi"]), [(q["tid"], q["beg"], q["end"]) for q in f["queries"]],
                    f["payload"] == 65280))
    for label, h, queries in Q.hand_cases():
        small = sum(len(c) for b in h.bins for c in b.values()) <= 6
        out.append(("hand " + label, TBI, h.tbi_raw(), h, queries + [(len(h.bins), 0, 10), (-1, 0, 10)], small))
        out.append(("hand, bai " + label, BAI, h.bai(), h, queries, small))
    bai, recs = Q.synthetic_bai()
    out.append(("synthetic bai", BAI, bai.bai(), bai, [(0, 0, 1 << 29), (0, 100000, 200000), (0, 1500000, 1500001)], False))
    no = Q.Hand(bai.bins, bai.linear, pseudo=(), n_no_coor=None)
    out.append(("synthetic bai without n_no_coor", BAI, no.bai(), no, [(0, 0, 1 << 29)], False))
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("index_query_host")
    exe = str(d / "driver")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", os.path.join(ROOT, "platypus_amd", "csrc"),
            os.path.join(ROOT, "tests", "index_query_host_driver.cpp"), "-o", exe]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan"], capture_output=True, text=True)
    if san.returncode != 0:
        subprocess.check_call(base)
    print("host driver built %s sanitizers" % ("with" if san.returncode == 0 else "WITHOUT"))
    return exe, d


@pytest.fixture(scope="module")
def twin(exe):
    """{label: {"rc", "n_ref", "no_coor", "tables", "names", "queries": [(rc, count, gathered, chunks)], "accepted": [lengths] or None}}"""
    exe, d = exe
    cases = all_indexes()
    fin, fout = str(d / "cases.in"), str(d / "cases.out")
    with open(fin, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for _, kind, raw, _, queries, prefixes in cases:
            f.write(struct.pack("<iiq", kind, int(prefixes), len(raw)) + raw + struct.pack("<i", len(queries)) + b"".join(struct.pack("<3i", *q) for q in queries))
    r = subprocess.run([exe, "cases", fin, fout], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    lines = open(fout).read().split("\n")
    out, at = {}, 0
    for label, _, _, _, queries, prefixes in cases:
        head = lines[at].split()
        assert head[0] == "I"
        e = dict(rc=int(head[1]), n_ref=int(head[2]), no_coor=int(head[3]), tables={}, names=[], queries=[], accepted=None)
        at += 1
        for _ in range(7):
            w = lines[at].split()
            e["tables"][w[1]] = [int(x) for x in w[2:]]
            at += 1
        while lines[at].startswith("N"):
            e["names"].append(bytes.fromhex(lines[at][2:]))
            at += 1
        for _ in queries:
            w = lines[at].split()
            assert w[0] == "Q"
            n = max(int(w[2]), 0)
            e["queries"].append((int(w[1]), int(w[2]), int(w[3]), [tuple(int(x) for x in lines[at + 1 + k].split()) for k in range(n)]))
            at += 1 + n
        if prefixes:
            assert lines[at].startswith("P")
            e["accepted"] = [int(x) for x in lines[at].split()[1:]]
            at += 1
        out[label] = e
    assert lines[at:] == [""]
    return out


def test_the_fixture_covers_what_it_should_and_pins_the_mirror():
    """Every recorded list is what TabixIndex.query returns; the queries cover both device paths and no query is beyond the limit."""
    files = Q.golden_files()
    assert [f["label"] for f in files] == ["wide", "dense"] and os.path.getsize(Q.GOLDEN) < 300 * 1024
    gathered = []
    for f in files:
        idx = tabixindex.TabixIndex(f["tbi"])
        for q in f["queries"]:
            assert idx.query(q["tid"], q["beg"], q["end"]) == q["chunks"], (f["label"], q["tid"], q["beg"], q["end"])
            gathered.append(Q.gathered_of(idx, q["tid"], q["beg"], q["end"]))
    assert any(q["chunks"] is None for f in files for q in f["queries"]) and any(q["chunks"] == [] for f in files for q in f["queries"])
    assert any(q["beg"] < 0 for f in files for q in f["queries"]) and any(q["end"] > 1 << 29 for f in files for q in f["queries"])
    assert min(gathered) == 0 and any(60 <= g <= 70 for g in gathered) and any(10 <= g <= 40 for g in gathered) and any(1400 <= g <= 1600 for g in gathered)
    assert max(gathered) <= Q.MAX_CHUNKS


def test_host_twin_flattens_to_the_mirrors_tables(twin):
    for label, kind, raw, index, queries, _ in all_indexes():
        e = twin[label]
        assert e["rc"] == 0, label
        assert e["tables"] == Q.flat_of(index), label
        assert e["n_ref"] == len(index.bins)
        if kind == TBI:
            assert e["names"] == list(index.names), label
        else:
            assert e["no_coor"] == (-1 if index.n_no_coor is None else index.n_no_coor), label


def test_host_twin_answers_as_the_reference_and_the_mirror(twin):
    n = 0
    for label, kind, raw, index, queries, _ in all_indexes():
        for q, (rc, count, gathered, chunks) in zip(queries, twin[label]["queries"]):
            if not 0 <= q[0] < len(index.bins):
                assert (rc, count, chunks) == (-1, 0, []), (label, q)
                continue
            want = index.query(*q)
            assert rc == 0 and (None if count == -1 else chunks) == want and count == (-1 if want is None else len(want)), (label, q)
            assert gathered == Q.gathered_of(index, *q), (label, q)
            n += 1
    assert n > 150
    for f in Q.golden_files():                                               # ... and the recorded lists themselves
        got = twin["fixture " + f["label"]]["queries"]
        assert [None if c == -1 else ch for _, c, _, ch in got] == [q["chunks"] for q in f["queries"]]


def test_every_prefix_is_refused_and_never_read_past(twin):
    """(The driver copies each prefix to a heap block of its own length: a read past it aborts under the sanitizer.)  A .bai's trailing
    n_no_coor is optional, so the prefixes that cut only it are indexes too."""
    seen = 0
    for label, kind, raw, index, _, prefixes in all_indexes():
        if not prefixes:
            continue
        seen += 1
        tail = 8 if kind == BAI and index.n_no_coor is not None else 0
        assert twin[label]["accepted"] == list(range(len(raw) - tail, len(raw))), label
    assert seen >= 6


def test_refusals_of_the_flatten(exe, tmp_path):
    exe, _ = exe
    h = Q.Hand([{4681: [(1 << 16, 2 << 16)], 585: [(3 << 16, 4 << 16)]}], [[5, 0, 7]])
    raw = h.tbi_raw()
    body = raw.index(struct.pack("<Ii", 585, 1))
    bad = {
        "a bin twice": raw[:body] + struct.pack("<I", 4681) + raw[body + 4:],
        "a bin above the pseudo-bin": raw[:body] + struct.pack("<I", 37451) + raw[body + 4:],
        "a negative chunk count": raw[:body + 4] + struct.pack("<i", -1) + raw[body + 8:],
        "a negative n_ref": raw[:4] + struct.pack("<i", -1) + raw[8:],
        "a bad magic": b"TBJ\x01" + raw[4:],
        "a chunk count beyond the bytes": raw[:body + 4] + struct.pack("<i", 1 << 30) + raw[body + 8:],
    }
    other = {"another preset": raw[:8] + struct.pack("<i", 0) + raw[12:], "too many references": raw[:4] + struct.pack("<i", 65537) + raw[8:]}
    fin, fout = str(tmp_path / "in"), str(tmp_path / "out")
    items = list(bad.items()) + list(other.items())
    with open(fin, "wb") as f:
        f.write(struct.pack("<I", len(items)) + b"".join(struct.pack("<iiq", TBI, 0, len(b)) + b + struct.pack("<i", 0) for _, b in items))
    r = subprocess.run([exe, "cases", fin, fout], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stderr[-2000:]
    rcs = [int(l.split()[1]) for l in open(fout).read().split("\n") if l.startswith("I")]
    assert rcs == [-9] * len(bad) + [-6] * len(other)


def test_the_parallel_restatement_equals_the_three_loops(exe):
    exe, _ = exe
    r = subprocess.run([exe, "loops", "20240607", "200000"], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stderr[-2000:]
    differ, n, chunks, ties, empty = map(int, r.stdout.split())
    assert differ == 0 and n == 200000 and ties > 10000 and empty > 100000
    # the same lists through the Python statement of the loops (tabixindex) and a plain restatement of the one scan
    for c in Q.random_lists(7, 3000):
        h = Q.Hand([{4681: c}], [[]])
        want = h.query(0, 0, 10)
        out, M = [], 0
        for i, (u, v) in enumerate(c):
            if i == 0 or (v > M and M >> 16 < u >> 16):
                if i:
                    out[-1] = (out[-1][0], M)
                out.append((u, v))
            M = max(M, v)
        if out:
            out[-1] = (out[-1][0], M)
        assert out == want, c


def test_bam_index_reader_reads_what_was_written():
    h, recs = Q.synthetic_bai()
    b = tabixindex.BamIndex(h.bai())
    assert b.bins == h.bins and b.linear == h.linear and b.n_no_coor == 17 and b.pseudo == [[(1, 2), (3, 4)]]
    assert tabixindex.BamIndex(Q.Hand(h.bins, h.linear).bai()).n_no_coor is None
    # every record overlapping a query starts inside a returned chunk: a property that needs no index rule
    for beg, end in ((0, 1 << 29), (100000, 200000), (1500000, 1500001), (2999000, 3100000), (5, 6)):
        chunks = b.query(0, beg, end)
        for rb, re_, u, v in recs:
            if rb < end and re_ > beg:
                assert any(cu <= u < cv for cu, cv in chunks), (beg, end, rb, re_)
    with pytest.raises(ValueError):
        tabixindex.BamIndex(b"BAM\x01")


def test_structs_match_their_ctypes_mirrors_and_the_symbol_is_declared(tmp_path):
    F.build()
    src = tmp_path / "lay.c"
    src.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include "platypus_mi355x.h"
#include "platypus_caller_index.h"
int main(void){
  printf("%zu %zu %zu %zu %zu %zu\n", sizeof(plat_index_query_in), sizeof(plat_index_query_out), offsetof(plat_index_query_in, n_bins), offsetof(plat_index_query_in, end),
         offsetof(plat_index_query_out, count), offsetof(plat_index_query_out, status));
  printf("%zu %zu %zu %zu %zu %zu\n", sizeof(plat_index_query_info), offsetof(plat_index_query_info, seconds), sizeof(plat_source_file), offsetof(plat_source_file, index),
         sizeof(plat_source_region), offsetof(plat_source_region, start));
  printf("%d %d %d %d %d %d\n", PLAT_IDXQ_STATUS_WORDS, PLAT_IDXQ_MAX_CHUNKS, PLAT_IDXQ_NO_ITERATOR, PLAT_IDXQ_HANDED_OVER, PLAT_INDEX_TBI, PLAT_INDEX_BAI);
  { int (*fn)(plat_ctx*, const plat_index_query_in*, const plat_index_query_out*, void*) = plat_index_query_batch; printf("%d\n", fn(NULL, NULL, NULL, NULL)); }
  { int (*fn)(plat_caller*, const plat_source_file*, int, const plat_source_region*, int, int, plat_source_blocks_info*) = plat_caller_set_source_files;
    printf("%d\n", fn(NULL, NULL, 0, NULL, 0, 0, NULL)); }
  return 0; }''')
    exe = tmp_path / "lay"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L" + os.path.dirname(F.LIB_PATH), "-lplat_caller",
                           "-lplat_mi355x", "-Wl,-rpath," + os.path.dirname(F.LIB_PATH)])
    vals = list(map(int, subprocess.check_output([str(exe)], text=True).split()))
    I, O = _lib.IndexQueryIn, _lib.IndexQueryOut
    assert vals[:6] == [C.sizeof(I), C.sizeof(O), I.n_bins.offset, I.end.offset, O.count.offset, O.status.offset]
    assert vals[6:12] == [C.sizeof(F.IndexQueryInfo), F.IndexQueryInfo.seconds.offset, C.sizeof(F._SourceFile), F._SourceFile.index.offset, C.sizeof(F._SourceRegion),
                          F._SourceRegion.start.offset]
    assert vals[12:18] == [_lib.IDXQ_STATUS_WORDS, _lib.IDXQ_MAX_CHUNKS, _lib.IDXQ_NO_ITERATOR, _lib.IDXQ_HANDED_OVER, F.INDEX_KINDS["tbi"], F.INDEX_KINDS["bai"]]
    assert vals[18:] == [-1, -1] and _lib.IDXQ_MAX_CHUNKS == Q.MAX_CHUNKS >= 2048
    assert "plat_index_query_batch" in _lib.SIGNATURES and "plat_index_query_batch" in _lib.ADDED_LATER and hasattr(_lib.load(), "plat_index_query_batch")
    assert "HOST_INDEX" in open(os.path.join(ROOT, "platypus_amd", "csrc", "host", "switches.hpp")).read()
    assert "plat_index_query_batch" in open(os.path.join(ROOT, "bindings", "cplat.pxd")).read()


def golden_regions(f):
    return [(f["names"][q["tid"]], q["beg"], q["end"]) for q in f["queries"]]


def test_fake_device_refuses_index_queries_and_stays_usable(monkeypatch):
    """The CPU stand-in device has no plat_index_query_batch: PLAT_ERR_UNSUPPORTED naming the symbol, twice, from both entry points."""
    from tests.fakedev import fake_caller_lib
    monkeypatch.delenv("PLAT_CALLER_HOST_INDEX", raising=False)
    nc = F.NativeCaller(0, 1, 1, lib=fake_caller_lib())
    try:
        f = T.golden_files()[1]
        idx = nc.open_index(f["tbi"])
        assert idx.n_refs == len(f["names"]) and [idx.ref_name(t) for t in range(idx.n_refs)] == f["names"] and idx.ref_name(idx.n_refs) is None
        assert [idx.tid(n) for n in f["names"]] == list(range(len(f["names"]))) and idx.tid(b"2_") == -1 and idx.tid(b"") == -1
        for _ in range(2):
            with pytest.raises(_lib.PlatypusDeviceError) as e:
                nc.query_index(idx, [(0, 0, 100)])
            assert e.value.code == -6 and "plat_index_query_batch" in str(e.value)
            with pytest.raises(_lib.PlatypusDeviceError) as e:
                nc.set_source_files([(f["vcf_gz"], idx)], golden_regions(f))
            assert e.value.code == -6 and "plat_index_query_batch" in str(e.value)
        with pytest.raises(_lib.PlatypusDeviceError) as e:
            nc.open_index(b"not an index")
        assert e.value.code == -9
        with pytest.raises(_lib.PlatypusDeviceError) as e:
            nc.open_index(f["tbi"], "bai")
        assert e.value.code == -9
        idx.close()
        assert nc.call_regions([], ["S1"], default_options()) == ""
    finally:
        nc.close()


def test_fake_device_host_index_takes_whole_files_and_returns_the_golden_lines(monkeypatch):
    """PLAT_CALLER_HOST_INDEX=1 and PLAT_CALLER_HOST_TABIX=1 on the stand-in device: over the three golden files, all 31 queries each,
    the golden lines -- and the text plat_caller_set_source_blocks sets from tabixindex's fetches, byte for byte."""
    from tests.fakedev import fake_caller_lib
    monkeypatch.setenv("PLAT_CALLER_HOST_INDEX", "1")
    monkeypatch.setenv("PLAT_CALLER_HOST_TABIX", "1")
    nc = F.NativeCaller(0, 1, 1, lib=fake_caller_lib())
    try:
        files = T.golden_files()
        assert len(files) == 3
        for f in files:
            idx = nc.open_index(f["tbi"])
            regions = golden_regions(f)
            assert len(regions) == 31
            got, info = nc.query_index(idx, [(q["tid"], q["beg"], q["end"]) for q in f["queries"]], info=True)
            mirror = tabixindex.TabixIndex(f["tbi"])
            assert got == [mirror.query(q["tid"], q["beg"], q["end"]) for q in f["queries"]]
            assert info["queries"] == info["handed_over"] == 31 and info["device_calls"] == 0
            # a name the index lacks and end < start leave the file out of their regions
            extra = regions + [(b"nope", 0, 100), (f["names"][0], 50, 10)]
            nc.set_source_files([(f["vcf_gz"], idx)], extra)
            by_files, info_files = nc.source_lines_set(len(extra)), nc.source_blocks_info
            for q, text in zip(f["queries"], by_files):
                assert text == b"".join(l + b"\n" for l in q["lines"]), (f["label"], q["tid"], q["beg"], q["end"])
            assert by_files[31:] == [b"", b""]
            tf = tabixindex.TabixFile(f["vcf_gz"], f["tbi"])
            nc.set_source_blocks([[b for b in [tf.fetch_blocks(*r)] if b is not None] for r in extra])
            assert nc.source_lines_set(len(extra)) == by_files
            assert {k: v for k, v in nc.source_blocks_info.items() if k != "seconds"} == {k: v for k, v in info_files.items() if k != "seconds"}
            # two files at once: the fetches of a region back to back in file order
            nc.set_source_files([(f["vcf_gz"], idx), (f["vcf_gz"], idx)], regions)
            assert nc.source_lines_set(31) == [t + t for t in by_files[:31]]
            # a chunk whose block is not in the data: named
            with pytest.raises(_lib.PlatypusDeviceError) as e:
                nc.set_source_files([(f["vcf_gz"][:30], idx)], regions[:12])
            assert e.value.code == -9 and "region" in str(e.value) and "file 0" in str(e.value) and "chunk" in str(e.value)
            # ... the file cut short behind its first block: the whole message, the offsets read off the file's own index
            cut = f["vcf_gz"][:struct.unpack_from("<H", f["vcf_gz"], 16)[0] + 1]
            with pytest.raises(_lib.PlatypusDeviceError) as e:
                nc.set_source_files([(f["vcf_gz"], idx), (cut, idx)], regions)
            bad = [(k, first_chunk_off_the_data(cut, mirror.query(q["tid"], q["beg"], q["end"]) or [])) for k, q in enumerate(f["queries"])]
            k, (n, u, v) = [b for b in bad if b[1] is not None][0]
            entry = "plat_caller_set_source_files"
            assert e.value.code == -9 and str(e.value) == str(_lib.PlatypusDeviceError(
                -9, "%s: chunk %d of region %d, file 1 (virtual offsets %d .. %d) %s" % (entry, n, k, u, v, NO_CUT), entry))
            with pytest.raises(_lib.PlatypusDeviceError) as e:
                nc.query_index(idx, [(0, 0, 5), (len(f["names"]), 0, 5)])
            assert e.value.code == -1 and "query 1" in str(e.value)
            nc.set_source_files([(f["vcf_gz"], idx)], [])
            with pytest.raises(_lib.PlatypusDeviceError):
                nc.source_lines_set(1)
            idx.close()
        assert nc.call_regions([], ["S1"], default_options()) == ""
    finally:
        nc.close()
