"""CPU tests of the raw-BAM-record region loop (include/platypus_caller_bam.h, plat_bam_decode_batch): the C structs match their ctypes
mirrors, the header compiles as C, the Cython declarations build, the caller library linked against the CPU stand-in device refuses the
call cleanly, and the record encoder (synth.bam_record) writes the bytes the SAM/BAM specification section 4.2 says -- three records
worked out by hand."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from platypus_amd import _lib, fastcaller as F, hostapi as H, synth
from platypus_amd.options import default_options

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bam_structs_match_their_ctypes_mirrors(tmp_path):
    F.build()
    src = tmp_path / "lay.c"
    src.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include "platypus_caller_bam.h"
#include "platypus_mi355x.h"
int main(void){
  printf("%zu %zu %zu %zu\n", sizeof(plat_bam_records), offsetof(plat_bam_records, data), offsetof(plat_bam_records, data_len),
         offsetof(plat_bam_records, rec_off));
  printf("%zu %zu\n", sizeof(plat_bam_sample), offsetof(plat_bam_sample, broken_mates));
  printf("%zu %zu %zu %zu\n", sizeof(plat_bam_region), offsetof(plat_bam_region, contig_seq), offsetof(plat_bam_region, samples),
         offsetof(plat_bam_region, dev_contig_seq));
  printf("%zu %zu %zu %zu %zu %zu\n", sizeof(plat_bam_decode_out), offsetof(plat_bam_decode_out, cap_pairs), offsetof(plat_bam_decode_out, read_off),
         offsetof(plat_bam_decode_out, cigar), offsetof(plat_bam_decode_out, chrom_id), offsetof(plat_bam_decode_out, status));
  { int (*fn)(plat_caller*, const plat_bam_region*, int, int, const char* const*, plat_caller_options*, const plat_caller_qc_options*, char**,
               size_t*, plat_fetched_region_info*, plat_caller_stats*) = plat_call_bam_regions;
    printf("%d\n", fn(NULL, NULL, 0, 0, NULL, NULL, NULL, NULL, NULL, NULL, NULL)); }
  return 0; }''')
    exe = tmp_path / "lay"
    # -std=c99 -pedantic-errors: the header is C, not only C++
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic-errors", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L" + os.path.dirname(F.LIB_PATH), "-lplat_caller", "-lplat_mi355x", "-Wl,-rpath," + os.path.dirname(F.LIB_PATH)])
    out = subprocess.check_output([str(exe)], text=True).split()
    v = list(map(int, out[:16]))
    R, S, G, D = F._BamRecords, F._BamSample, F._BamRegion, _lib.BamDecodeOut
    assert v[0:4] == [C.sizeof(R), R.data.offset, R.data_len.offset, R.rec_off.offset]
    assert v[4:6] == [C.sizeof(S), S.broken_mates.offset]
    assert v[6:10] == [C.sizeof(G), G.contig_seq.offset, G.samples.offset, G.dev_contig_seq.offset]
    assert v[10:16] == [C.sizeof(D), D.cap_pairs.offset, D.read_off.offset, D.cigar.offset, D.chrom_id.offset, D.status.offset]
    assert int(out[16]) == -1                                # (PLAT_ERR_INVALID for a NULL caller: the symbol links and runs)
    # the device entry point is declared, bound and exported
    assert "plat_bam_decode_batch" in _lib.SIGNATURES and hasattr(_lib.load(), "plat_bam_decode_batch")
    assert len(_lib.SIGNATURES["plat_bam_decode_batch"][1]) == 8


def test_cython_declarations_of_the_bam_entry_points_build(tmp_path):
    pytest.importorskip("Cython")
    pyx = tmp_path / "bam_check.pyx"
    pyx.write_text('''# cython: language_level=3
from libc.string cimport memset
cimport cplat

def sizes():
    cdef cplat.plat_bam_region r
    cdef cplat.plat_bam_decode_out o
    memset(&r, 0, sizeof(r))
    memset(&o, 0, sizeof(o))
    return (sizeof(cplat.plat_bam_records), sizeof(cplat.plat_bam_sample), sizeof(r), sizeof(o),
            cplat.plat_bam_decode_batch(NULL, 0, NULL, 0, NULL, NULL, &o, NULL),
            cplat.plat_call_bam_regions(NULL, &r, 0, 0, NULL, NULL, NULL, NULL, NULL, NULL, NULL))
''')
    c_file = tmp_path / "bam_check.c"
    subprocess.check_call([sys.executable, "-m", "cython", "-3", "-I", os.path.join(ROOT, "bindings"), str(pyx), "-o", str(c_file)])
    import sysconfig
    obj = tmp_path / "bam_check.o"
    subprocess.check_call(["gcc", "-c", "-fPIC", "-O0", "-I" + sysconfig.get_paths()["include"], "-I" + os.path.join(ROOT, "include"), str(c_file),
                           "-o", str(obj)])


def _tiny_region():
    ref = b"ACGT" * 100
    fasta = H.FastaFile({"20": ref})
    reads = [H.AlignedRead(ref[p:p + 50], bytes([30] * 50), p, bitFlag=3) for p in (110, 120)]
    return F.BamRegion.from_reads("20", 100, 300, fasta, [(reads, [])])


def test_fake_device_caller_library_refuses_the_bam_call_and_stays_usable():
    """The CPU stand-in device has no plat_bam_decode_batch: the caller library still loads, returns PLAT_ERR_UNSUPPORTED with a message, and
    works afterwards."""
    from tests.fakedev import fake_caller_lib
    lib = fake_caller_lib()
    nc = F.NativeCaller(0, 1, 1, lib=lib)
    try:
        for _ in range(2):
            with pytest.raises(_lib.PlatypusDeviceError) as e:
                nc.call_bam_regions([_tiny_region()], ["S1"], default_options())
            assert e.value.code == -6 and "plat_bam_decode_batch" in str(e.value)
        assert nc.call_regions([], ["S1"], default_options()) == ""
    finally:
        nc.close()


def test_fake_engine_still_binds_without_the_decode():
    from tests.fakedev import fake_engine
    eng = fake_engine()
    assert not hasattr(eng.lib, "plat_bam_decode_batch") or eng.lib.plat_bam_decode_batch.argtypes
    assert eng.lib.plat_read_qc_batch.argtypes


def test_encoder_writes_the_specified_bytes():
    """Three records by hand (SAM/BAM specification 4.2: core from refID on, read_name, cigar words len << 4 | op, 4-bit bases high nibble
    first in "=ACMGRSVTWYHKDBN", qualities, aux)."""
    # 1: the plain case -- 20:100, 4M, ACGT
    r1 = H.AlignedRead(b"ACGT", bytes([30, 31, 32, 33]), 100, 60, 3, cigarOps=[(0, 4)], chromID=0, mateChromID=0, insertSize=104, matePos=200)
    assert synth.bam_record(r1, b"a\0").hex() == (
        "00000000" "64000000" "02" "3c" "0000" "0100" "0300" "04000000" "00000000" "c8000000" "68000000"
        "6100" "40000000" "1248" "1e1f2021")
    # 2: a leading soft clip (the read's pos 995 is the record's 1000 - 5), an odd length (last low nibble 0), '=' and N, qualities 0 / 93 /
    #    254, negative mate fields and insert size, a three-byte name and aux data
    r2 = H.AlignedRead(b"=NACGTM", bytes([0, 93, 254, 1, 2, 3, 4]), 995, 0, 0x451, cigarOps=[(4, 5), (0, 2)], chromID=19, mateChromID=-1,
                       insertSize=-300, matePos=-1)
    assert synth.bam_record(r2, b"q1\0", b"XYZ").hex() == (
        "13000000" "e8030000" "03" "00" "0000" "0200" "5104" "07000000" "ffffffff" "ffffffff" "d4feffff"
        "713100" "54000000" "20000000" "0f124830" "005dfe01020304" "58595a")
    # 3: unmapped, no CIGAR, one base, a one-byte name, bin in its place
    r3 = H.AlignedRead(b"T", bytes([40]), -1, 255, 4, cigarOps=[], chromID=-1, mateChromID=-1, insertSize=0, matePos=-1)
    assert synth.bam_record(r3, b"\0", bin_=0x1248).hex() == (
        "ffffffff" "ffffffff" "01" "ff" "4812" "0000" "0400" "01000000" "ffffffff" "ffffffff" "00000000"
        "00" "80" "28")
    # back to back, with block_size words and bytes in front
    data, off = synth.bam_records([r1, r3], names=[b"a\0", b"\0"], lead=3, block_size=True)
    n1 = len(synth.bam_record(r1, b"a\0"))
    assert list(off) == [7, 7 + n1 + 4] and len(data) == 3 + 4 + n1 + 4 + 35
    assert data[3:7].tobytes() == n1.to_bytes(4, "little") and data[7 + n1:11 + n1].tobytes() == (35).to_bytes(4, "little")
    assert data[7:7 + n1].tobytes() == synth.bam_record(r1, b"a\0")
    # what no record can hold is refused by the encoder
    for bad in (H.AlignedRead(b"ACGU", bytes(4), 0), H.AlignedRead(b"", b"", 0)):
        with pytest.raises(ValueError):
            synth.bam_record(bad)
    assert isinstance(data, np.ndarray) and off.dtype == np.int64
