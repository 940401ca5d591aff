"""CPU tests of the read-group front ends (plat_bam_route_batch, include/platypus_caller_rg.h): the C structs match their ctypes mirrors,
the new header compiles as C, the Cython declarations build, the caller library linked against the CPU stand-in device refuses both new
calls cleanly, and the HOST BUILD of csrc/bam_aux.hpp -- the code that indexes memory from record bytes, the same text the device compiles
-- gives the verdict and the sample of the rule restated in tests/bam_aux_reference.py on the hand-made records, on every truncation of a
200-byte record and on 2 000 single-byte mutations of its aux area, each record in a heap block of exactly its size (under
AddressSanitizer and UBSan where libasan is installed)."""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from platypus_amd import _lib, fastcaller as F, hostapi as H
from platypus_amd.options import default_options
from tests import bam_aux_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_read_group_structs_match_their_ctypes_mirrors(tmp_path):
    F.build()
    src = tmp_path / "lay.c"
    src.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include "platypus_caller_rg.h"
#include "platypus_mi355x.h"
int main(void){
  printf("%zu %zu %zu\n", sizeof(plat_bam_read_groups), offsetof(plat_bam_read_groups, id), offsetof(plat_bam_read_groups, sample));
  printf("%zu %zu %zu %zu\n", sizeof(plat_bam_file_records), offsetof(plat_bam_file_records, rec_len), sizeof(plat_bam_file),
         offsetof(plat_bam_file, broken_mates));
  printf("%zu %zu %zu\n", sizeof(plat_bgzf_file), offsetof(plat_bgzf_file, chunks), offsetof(plat_bgzf_file, broken_mates));
  printf("%zu %zu %zu %zu\n", sizeof(plat_bam_rg_region), offsetof(plat_bam_rg_region, contig_seq), offsetof(plat_bam_rg_region, files),
         offsetof(plat_bam_rg_region, dev_contig_seq));
  printf("%zu %zu %zu %zu\n", sizeof(plat_bgzf_rg_region), offsetof(plat_bgzf_rg_region, dev_contig_seq), offsetof(plat_bgzf_rg_region, tid),
         offsetof(plat_bgzf_rg_region, files));
  printf("%zu %zu %zu %zu %zu %zu\n", sizeof(plat_bam_route_in), offsetof(plat_bam_route_in, n_samples), offsetof(plat_bam_route_in, blob),
         offsetof(plat_bam_route_in, blob_len), offsetof(plat_bam_route_in, stream_begin), offsetof(plat_bam_route_in, group_sample));
  printf("%zu %zu %zu %zu\n", sizeof(plat_bam_route_out), offsetof(plat_bam_route_out, out_begin), offsetof(plat_bam_route_out, status),
         offsetof(plat_bam_route_out, why));
  printf("%d %d %d %d %d\n", PLAT_ROUTE_MAX_GROUPS, PLAT_ROUTE_MAX_SAMPLES, PLAT_ROUTE_LDS_ID_BYTES, PLAT_ROUTE_NO_RG, PLAT_ROUTE_FIXED_OVERRUN);
  { int (*fn)(plat_caller*, const plat_bam_rg_region*, int, int, const plat_bam_read_groups*, int, const char* const*, plat_caller_options*,
               const plat_caller_qc_options*, char**, size_t*, plat_fetched_region_info*, plat_caller_stats*) = plat_call_bam_regions_rg;
    int (*gn)(plat_caller*, const plat_bgzf_rg_region*, int, int, const plat_bam_read_groups*, int, const char* const*, plat_caller_options*,
               const plat_caller_qc_options*, char**, size_t*, plat_fetched_region_info*, plat_caller_stats*) = plat_call_bgzf_regions_rg;
    printf("%d %d\n", fn(NULL, NULL, 0, 1, NULL, 1, NULL, NULL, NULL, NULL, NULL, NULL, NULL),
           gn(NULL, NULL, 0, 1, NULL, 1, NULL, NULL, NULL, NULL, NULL, NULL, NULL)); }
  return 0; }''')
    exe = tmp_path / "lay"
    # -std=c99 -pedantic-errors: the header is C, not only C++
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic-errors", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L" + os.path.dirname(F.LIB_PATH), "-lplat_caller", "-lplat_mi355x", "-Wl,-rpath," + os.path.dirname(F.LIB_PATH)])
    out = list(map(int, subprocess.check_output([str(exe)], text=True).split()))
    G, FR, FL, BF, A, B, RI, RO = (F._BamReadGroups, F._BamFileRecords, F._BamFile, F._BgzfFile, F._BamRgRegion, F._BgzfRgRegion, _lib.BamRouteIn,
                                   _lib.BamRouteOut)
    assert out[0:3] == [C.sizeof(G), G.id.offset, G.sample.offset]
    assert out[3:7] == [C.sizeof(FR), FR.rec_len.offset, C.sizeof(FL), FL.broken_mates.offset]
    assert out[7:10] == [C.sizeof(BF), BF.chunks.offset, BF.broken_mates.offset]
    assert out[10:14] == [C.sizeof(A), A.contig_seq.offset, A.files.offset, A.dev_contig_seq.offset]
    assert out[14:18] == [C.sizeof(B), B.dev_contig_seq.offset, B.tid.offset, B.files.offset]
    assert out[18:24] == [C.sizeof(RI), RI.n_samples.offset, RI.blob.offset, RI.blob_len.offset, RI.stream_begin.offset, RI.group_sample.offset]
    assert out[24:28] == [C.sizeof(RO), RO.out_begin.offset, RO.status.offset, RO.why.offset]
    assert out[28:33] == [_lib.ROUTE_MAX_GROUPS, _lib.ROUTE_MAX_SAMPLES, _lib.ROUTE_LDS_ID_BYTES, R.NO_RG, R.FIXED_OVERRUN]
    assert out[33:35] == [-1, -1]                            # (PLAT_ERR_INVALID for a NULL caller: the symbols link and run)
    assert _lib.ROUTE_MAX_GROUPS >= 1024 and _lib.ROUTE_MAX_SAMPLES >= 128 and len(_lib.ROUTE_WHY) == len(R.REASONS) == 8
    # the device entry point is declared, bound and exported
    assert "plat_bam_route_batch" in _lib.SIGNATURES and hasattr(_lib.load(), "plat_bam_route_batch")
    assert len(_lib.SIGNATURES["plat_bam_route_batch"][1]) == 4
    # the two record headers' closing lines point here
    for h in ("platypus_caller_bam.h", "platypus_caller_bgzf.h"):
        with open(os.path.join(ROOT, "include", h)) as f:
            assert "platypus_caller_rg.h" in f.read(), h


def test_cython_declarations_of_the_read_group_entry_points_build(tmp_path):
    pytest.importorskip("Cython")
    pyx = tmp_path / "rg_check.pyx"
    pyx.write_text('''# cython: language_level=3
from libc.string cimport memset
cimport cplat

def sizes():
    cdef cplat.plat_bam_rg_region r
    cdef cplat.plat_bgzf_rg_region g
    cdef cplat.plat_bam_route_in qi
    cdef cplat.plat_bam_route_out qo
    cdef cplat.plat_bam_read_groups t
    memset(&r, 0, sizeof(r))
    memset(&g, 0, sizeof(g))
    memset(&qi, 0, sizeof(qi))
    memset(&qo, 0, sizeof(qo))
    memset(&t, 0, sizeof(t))
    return (sizeof(cplat.plat_bam_file_records), sizeof(cplat.plat_bam_file), sizeof(cplat.plat_bgzf_file), sizeof(r), sizeof(g),
            cplat.PLAT_ROUTE_MAX_GROUPS, cplat.plat_bam_route_batch(NULL, &qi, &qo, NULL),
            cplat.plat_call_bam_regions_rg(NULL, &r, 0, 1, &t, 1, NULL, NULL, NULL, NULL, NULL, NULL, NULL),
            cplat.plat_call_bgzf_regions_rg(NULL, &g, 0, 1, &t, 1, NULL, NULL, NULL, NULL, NULL, NULL, NULL))
''')
    c_file = tmp_path / "rg_check.c"
    subprocess.check_call([sys.executable, "-m", "cython", "-3", "-I", os.path.join(ROOT, "bindings"), str(pyx), "-o", str(c_file)])
    import sysconfig
    subprocess.check_call(["gcc", "-c", "-fPIC", "-O0", "-I" + sysconfig.get_paths()["include"], "-I" + os.path.join(ROOT, "include"), str(c_file),
                           "-o", str(tmp_path / "rg_check.o")])


def _tiny_files():
    ref = b"ACGT" * 100
    fasta = H.FastaFile({"20": ref})
    rd = lambda p: H.AlignedRead(ref[p:p + 50], bytes([30] * 50), p, bitFlag=3)
    return fasta, [[(0, "lane1", [rd(110), rd(130)], []), (1, "lane2", [rd(120)], [])]]


def test_merged_file_is_interleaved_by_position_with_its_read_groups():
    fasta, files = _tiny_files()
    reg = F.BamFileRegion.from_reads("20", 100, 300, fasta, files)
    (data, off, ln), (bdata, boff, bln) = reg.files[0]
    recs = [data[o:o + n].tobytes() for o, n in zip(off, ln)]
    assert [struct.unpack_from("<i", r, 4)[0] for r in recs] == [110, 120, 130]
    table = {b"lane1": 0, b"lane2": 1}
    assert [R.verdict(r, table) for r in recs] == [(R.ROUTED, 0), (R.ROUTED, 1), (R.ROUTED, 0)]
    assert [r[-9:] for r in recs] == [b"RGZlane1\0", b"RGZlane2\0", b"RGZlane1\0"] and len(boff) == 0 and len(bln) == 0
    assert sum(ln) == len(data) and reg.record_bytes == len(data)
    g = F.BgzfFileRegion.from_reads("20", 100, 300, fasta, files)
    assert len(g.files) == 1 and len(g.files[0][0]) == 1 and g.compressed_bytes > 28


def test_fake_device_caller_library_refuses_the_read_group_calls_and_stays_usable():
    """The CPU stand-in device has no plat_bam_route_batch: the caller library still loads, returns PLAT_ERR_UNSUPPORTED with a message naming
    the symbol, twice per call, and works afterwards."""
    from tests.fakedev import fake_caller_lib
    lib = fake_caller_lib()
    nc = F.NativeCaller(0, 1, 1, lib=lib)
    fasta, files = _tiny_files()
    groups = {"lane1": 0, "lane2": 1}
    try:
        for _ in range(2):
            with pytest.raises(_lib.PlatypusDeviceError) as e:
                nc.call_bam_regions_rg([F.BamFileRegion.from_reads("20", 100, 300, fasta, files)], groups, ["S1", "S2"], default_options())
            assert e.value.code == -6 and "plat_bam_route_batch" in str(e.value)
            with pytest.raises(_lib.PlatypusDeviceError) as e:
                nc.call_bgzf_regions_rg([F.BgzfFileRegion.from_reads("20", 100, 300, fasta, files)], groups, ["S1", "S2"], default_options())
            assert e.value.code == -6 and "plat_bam_route_batch" in str(e.value)
        assert nc.call_regions([], ["S1"], default_options()) == ""
    finally:
        nc.close()


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """tests/bam_aux_host_driver.cpp + csrc/bam_aux.hpp built with g++, with -fsanitize=address,undefined when that links here."""
    d = tmp_path_factory.mktemp("bam_aux_host")
    exe = str(d / "driver")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", os.path.join(ROOT, "platypus_amd", "csrc"),
            os.path.join(ROOT, "tests", "bam_aux_host_driver.cpp"), "-o", exe]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan"], capture_output=True, text=True)
    sanitized = san.returncode == 0
    if not sanitized:
        subprocess.check_call(base)
    print("host driver built %s sanitizers" % ("with" if sanitized else "WITHOUT"))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0")     # (a library loaded in front of ASan's runtime is no error)

    def run(ids, samples, records, tag, lead=0):
        fin, fout = str(d / (tag + ".in")), str(d / (tag + ".out"))
        with open(fin, "wb") as f:
            f.write(struct.pack("<I", len(ids)))
            for i, s in zip(ids, samples):
                f.write(struct.pack("<I", len(i)) + i + struct.pack("<i", s))
            f.write(struct.pack("<I", len(records)))
            for r in records:
                f.write(struct.pack("<II", lead, len(r)) + r)
        r = subprocess.run([exe, fin, fout], capture_output=True, text=True, env=env)
        assert r.returncode == 0, (r.returncode, r.stderr[-3000:])       # a sanitizer report, a read outside a record, or an abort
        raw = np.fromfile(fout, dtype=np.int32).reshape(-1, 2)
        assert len(raw) == len(records)
        return [(int(a), int(b)) for a, b in raw]
    return run


def test_host_build_gives_the_rule_on_the_hand_made_records(driver):
    cases = R.hand_records()
    table = R.table_of(R.IDS, R.SAMPLES)
    want = [R.verdict(rec, table) for _, rec in cases]
    for lead in (0, 3):
        got = driver(R.IDS, R.SAMPLES, [rec for _, rec in cases], "hand%d" % lead, lead)
        assert [name for (name, _), g, w in zip(cases, got, want) if g != w] == []
    by = dict(zip([n for n, _ in cases], want))
    # what the rule gives, by hand
    assert by["RG first"] == by["an ID that is a prefix of another"] == (R.ROUTED, 0)       # (grpA is listed twice: its first entry counts)
    assert by["RG last"] == by["the longer of the two"] == (R.ROUTED, 1) and by["RG alone, type H"] == (R.ROUTED, 1)
    assert by["duplicate RG: the first decides"] == (R.ROUTED, 2) and by["duplicate RG: the first is unknown"] == (R.NOT_IN_TABLE, -1)
    assert by["RG of type i"] == by["RG of type A behind a field"] == (R.RG_NOT_STRING, -1)
    assert by["an empty value"] == by["a prefix of an ID"] == by["an ID with a byte more"] == (R.NOT_IN_TABLE, -1)
    assert by["no aux data"] == by["no RG field"] == by["two stray bytes behind the last field"] == by["the fixed part ends with the record"] == (R.NO_RG, -1)
    assert by["unknown type"] == by["unknown B subtype"] == (R.UNKNOWN_TYPE, -1) and by["negative B count"] == (R.NEGATIVE_COUNT, -1)
    for name in ("B count past the end", "B header cut", "Z without NUL", "RG without NUL", "i cut"):
        assert by[name] == (R.AUX_OVERRUN, -1), name
    for name in ("the qualities are cut", "31 bytes", "l_seq negative"):
        assert by[name] == (R.FIXED_OVERRUN, -1), name
    assert by["a long name and three CIGAR words"] == (R.ROUTED, 1) and by["an odd number of bases and no CIGAR"] == (R.ROUTED, 2)
    # RG behind each of the twelve field types and each B subtype is found
    behind = [w for (n, _), w in zip(cases, want) if n.startswith("RG behind")]
    assert len(behind) == 12 + 8 and all(v == R.ROUTED for v, _ in behind)
    assert set(v for v, _ in want) == set(range(8))                  # every verdict occurs
    # 300 groups, two and three IDs per sample, IDs of 1 to 255 bytes: every group's own record finds its sample
    rng = np.random.default_rng(11)
    ids = sorted({bytes(rng.integers(33, 127, size=int(n), dtype=np.uint8)) for n in rng.integers(1, 256, size=330)})[:300]
    samples = [(g // 2) % 130 for g in range(300)]
    recs = [R.fixed_part() + R.TWELVE[g % 12] + R.rg(i) for g, i in enumerate(ids)]
    assert driver(ids, samples, recs, "many") == [(R.ROUTED, s) for s in samples]
    assert driver([], [], recs[:3], "empty") == [(R.NOT_IN_TABLE, -1)] * 3


def test_host_build_gives_the_rule_on_every_truncation_and_2000_mutations(driver):
    rec, aux_at = R.record_200()
    table = R.table_of(R.IDS, R.SAMPLES)
    assert R.verdict(rec, table) == (R.ROUTED, 1)
    cuts = [rec[:k] for k in range(201)]
    want = [R.verdict(c, table) for c in cuts]
    assert driver(R.IDS, R.SAMPLES, cuts, "cuts") == want
    assert want[:aux_at] == [(R.FIXED_OVERRUN, -1)] * aux_at and want[aux_at] == (R.NO_RG, -1) and want[200] == (R.ROUTED, 1)
    assert {v for v, _ in want[aux_at:]} == {R.NO_RG, R.AUX_OVERRUN, R.ROUTED}
    rng = np.random.default_rng(2025)
    mutated = []
    for _ in range(2000):
        b = bytearray(rec)
        at = int(rng.integers(aux_at, 200))
        b[at] = (b[at] + int(rng.integers(1, 256))) & 0xff
        mutated.append(bytes(b))
    want = [R.verdict(m, table) for m in mutated]
    got = driver(R.IDS, R.SAMPLES, mutated, "mutations")
    assert [k for k in range(2000) if got[k] != want[k]] == []
    seen = {v for v, _ in want}
    print("mutations: verdicts", sorted(seen), "routed", sum(1 for v, _ in want if v == R.ROUTED))
    assert {R.ROUTED, R.NO_RG, R.NOT_IN_TABLE, R.UNKNOWN_TYPE, R.AUX_OVERRUN} <= seen
