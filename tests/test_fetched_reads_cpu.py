"""CPU tests of the fetched-reads region loop (include/platypus_caller_fetched.h, plat_read_buffers_batch): the C structs match their
ctypes mirrors, the caller library linked against the CPU stand-in device still loads and refuses the call cleanly, and the refusal
rules of the Python mirror hostapi.bamReadBuffer.fromFetchedReads (which need no device)."""
import ctypes as C
import os
import subprocess

import pytest

from platypus_amd import _lib, fastcaller as F, hostapi as H
from platypus_amd.options import default_options

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fetched_structs_match_their_ctypes_mirrors(tmp_path):
    F.build()
    src = tmp_path / "lay.c"
    src.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include "platypus_caller_fetched.h"
#include "platypus_mi355x.h"
int main(void){
  printf("%zu %zu %zu %zu\n", sizeof(plat_fetched_reads), offsetof(plat_fetched_reads, broken_mates), offsetof(plat_fetched_reads, chrom_id),
         offsetof(plat_fetched_reads, insert_size));
  printf("%zu %zu %zu\n", sizeof(plat_fetched_region), offsetof(plat_fetched_region, samples), offsetof(plat_fetched_region, dev_contig_seq));
  printf("%zu %zu %zu %zu\n", sizeof(plat_caller_qc_options), offsetof(plat_caller_qc_options, trimOverlapping),
         sizeof(plat_fetched_region_info), offsetof(plat_fetched_region_info, sample_counts));
  printf("%zu %zu %zu %zu %zu\n", sizeof(plat_read_buffers_in), offsetof(plat_read_buffers_in, n_streams), offsetof(plat_read_buffers_in, read_end),
         sizeof(plat_read_buffers_tables), offsetof(plat_read_buffers_tables, mate_pos));
  plat_caller_qc_options q; plat_caller_default_qc_options(&q);
  printf("%d %d %d %d %d %d %d %d %d %d %d\n", q.minGoodQualBases, q.minMapQual, q.minBaseQual, q.trimOverlapping, q.trimAdapter, q.trimReadFlank,
         q.trimSoftClipped, q.filterDuplicates, q.filterReadsWithUnmappedMates, q.filterReadsWithDistantMates, q.filterReadPairsWithSmallInserts);
  return 0; }''')
    exe = tmp_path / "lay"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L" + os.path.dirname(F.LIB_PATH), "-lplat_caller",
                           "-lplat_mi355x", "-Wl,-rpath," + os.path.dirname(F.LIB_PATH)])
    v = list(map(int, subprocess.check_output([str(exe)], text=True).split()))
    FR, FG, Q, I = F._FetchedReads, F._FetchedRegion, F.CallerQCOptions, F._FetchedRegionInfo
    assert v[0:4] == [C.sizeof(FR), FR.broken_mates.offset, FR.chrom_id.offset, FR.insert_size.offset]
    assert v[4:7] == [C.sizeof(FG), FG.samples.offset, FG.dev_contig_seq.offset]
    assert v[7:11] == [C.sizeof(Q), Q.trimOverlapping.offset, C.sizeof(I), I.sample_counts.offset]
    RI, RT = _lib.ReadBuffersIn, _lib.ReadBuffersTables
    assert v[11:16] == [C.sizeof(RI), RI.n_streams.offset, RI.read_end.offset, C.sizeof(RT), RT.mate_pos.offset]
    q = Q.from_options(default_options())                       # the defaults of runner.py, as the options object holds them
    assert v[16:] == [getattr(q, k) for k, _ in Q._fields_]


def _tiny_region(unsorted=False):
    ref = b"ACGT" * 100
    fasta = H.FastaFile({"20": ref})
    pos = [120, 110] if unsorted else [110, 120]
    reads = [H.AlignedRead(ref[p:p + 50], bytes([30] * 50), p, bitFlag=3) for p in pos]
    return F.FetchedRegion.from_reads("20", 100, 300, fasta, [(reads, [])])


def test_fake_device_caller_library_loads_and_refuses_the_fetched_call():
    """The CPU stand-in device has no plat_read_buffers_batch: the caller library still loads (RTLD_NOW), returns PLAT_ERR_UNSUPPORTED with a
    message, and stays usable."""
    from tests.fakedev import fake_caller_lib
    lib = fake_caller_lib()
    nc = F.NativeCaller(0, 1, 1, lib=lib)
    try:
        for _ in range(2):
            with pytest.raises(_lib.PlatypusDeviceError) as e:
                nc.call_fetched_regions([_tiny_region()], ["S1"], default_options())
            assert e.value.code == -6 and "plat_read_buffers_batch" in str(e.value)
        assert nc.call_regions([], ["S1"], default_options()) == ""
    finally:
        nc.close()


def test_fake_engine_still_binds():
    """The stand-in device library lacks the new entry point; binding it leaves that one unbound and everything else bound."""
    from tests.fakedev import fake_engine
    eng = fake_engine()
    assert not hasattr(eng.lib, "plat_read_buffers_batch") or eng.lib.plat_read_buffers_batch.argtypes
    assert eng.lib.plat_read_qc_batch.argtypes


def test_from_fetched_reads_refuses_unsorted_input():
    reads = [H.AlignedRead(b"A" * 40, bytes([30] * 40), p) for p in (100, 105, 103)]
    with pytest.raises(ValueError, match="not sorted"):
        H.bamReadBuffer.fromFetchedReads(reads, options=default_options())


def test_from_fetched_reads_gives_up_at_max_reads():
    """loadBAMData returns None once `totalReads >= maxReads` (platypusutils.pyx:538-541), counting over the region's samples."""
    reads = [H.AlignedRead(b"A" * 40, bytes([30] * 40), 100 + p) for p in range(5)]
    assert H.bamReadBuffer.fromFetchedReads(reads, options=default_options(maxReads=5)) is None
    assert H.bamReadBuffer.fromFetchedReads(reads, options=default_options(maxReads=8), readsBefore=3) is None
    assert H.bamReadBuffer.fromFetchedReads(reads[:2], options=default_options(maxReads=1), readsBefore=7) is None
    # a sample without reads never reaches the test; nothing is asked of the device
    b = H.bamReadBuffer.fromFetchedReads([], [], options=default_options(maxReads=0), readsBefore=9)
    assert b is not None and b.reads.getSize() == 0 and b.badReads.getSize() == 0
    off = default_options(maxReads=0, filterDuplicates=0)
    assert H.bamReadBuffer.fromFetchedReads([], options=off).filteredReadCountsByType == [0, 0, 0, 0, 0, -1, 0]
