"""CPU tests of packed fetched reads (plat_read_buffers_packed_batch, PLAT_READS_PACKED tables for plat_call_fetched_regions): the new
struct matches its ctypes mirror, the caller library linked against the CPU stand-in device still loads and refuses a packed call cleanly,
and FetchedRegion.from_reads(packed=True) hands over tables that decode to the reads' bytes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from platypus_amd import _lib, fastcaller as F, hostapi as H
from platypus_amd.options import default_options

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_packed_in_struct_matches_its_ctypes_mirror(tmp_path):
    src = tmp_path / "lay.c"
    src.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include "platypus_mi355x.h"
int main(void){
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(plat_read_buffers_packed_in), offsetof(plat_read_buffers_packed_in, qc),
         offsetof(plat_read_buffers_packed_in, n_streams), offsetof(plat_read_buffers_packed_in, stream_begin),
         offsetof(plat_read_buffers_packed_in, read_packed), offsetof(plat_read_buffers_packed_in, read_end),
         offsetof(plat_read_buffers_packed_in, n_exc), offsetof(plat_read_buffers_packed_in, exc_index),
         offsetof(plat_read_buffers_packed_in, exc_base), offsetof(plat_read_buffers_packed_in, exc_qual));
  return 0; }''')
    exe = tmp_path / "lay"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    v = list(map(int, subprocess.check_output([str(exe)], text=True).split()))
    P = _lib.ReadBuffersPackedIn
    assert v == [C.sizeof(P)] + [getattr(P, k).offset for k in ("qc", "n_streams", "stream_begin", "read_packed", "read_end", "n_exc", "exc_index",
                                                                 "exc_base", "exc_qual")]
    assert "plat_read_buffers_packed_batch" in _lib.SIGNATURES and "plat_read_buffers_packed_batch" in _lib.ADDED_LATER


def _reads_with_exceptions():
    ref = b"ACGTTGCAAGCT" * 40
    reads = []
    for k, p in enumerate((100, 110, 130, 170)):
        seq, qual = bytearray(ref[p:p + 50]), bytearray(range(10, 60))
        if k == 0:
            seq[0], qual[49] = ord("N"), 64                   # first byte of the blob, a quality just above the packed range
        if k == 2:
            seq[7], qual[8], qual[20] = ord("R"), 127, 200
        if k == 3:
            seq[49], qual[49] = ord("N"), 255                 # last byte of the blob
        reads.append(H.AlignedRead(bytes(seq), bytes(qual), p, bitFlag=3))
    return H.FastaFile({"20": ref}), reads


def _decode(t):
    n = t.n
    nb = int(t.off[n]) if n else 0
    packed = t.seq[:nb]
    seq = np.frombuffer(b"ACTG", dtype=np.uint8)[packed & 3]
    qual = (packed >> 2).astype(np.uint8)
    ix, eb, eq = t.exc
    seq[ix], qual[ix] = eb, eq
    return seq.tobytes(), qual.tobytes()


def test_from_reads_packed_decodes_to_the_input_bytes():
    fasta, reads = _reads_with_exceptions()
    broken = [H.AlignedRead(b"ACGNA" * 10, bytes([70] * 50), 300, matePos=m) for m in (500, 400)]
    reg = F.FetchedRegion.from_reads("20", 100, 300, fasta, [(reads, broken)], packed=True)
    f, b, cid, mcid, ins = reg.samples[0]
    assert f.encoding == F.READS_PACKED and b.encoding == F.READS_PACKED
    assert _decode(f) == (b"".join(r.seq for r in reads), b"".join(r.qual for r in reads))
    assert list(f.exc[0]) == [0, 49, 107, 108, 120, 199]
    assert _decode(b) == (b"".join(r.seq for r in sorted(broken, key=lambda r: r.matePos)), bytes([70] * 100))
    s = f.struct()
    assert s.encoding == F.READS_PACKED and s.n_exceptions == 6 and s.exc_index
    plain = F.FetchedRegion.from_reads("20", 100, 300, fasta, [(reads, broken)])
    assert plain.samples[0][0].encoding == F.READS_ASCII and plain.samples[0][0].exc is None


def test_fake_device_caller_library_refuses_the_packed_call():
    """The CPU stand-in device has neither read-buffer entry point: the caller library still loads, a packed fetched call returns
    PLAT_ERR_UNSUPPORTED with a message, and the caller stays usable."""
    from tests.fakedev import fake_caller_lib
    fasta, reads = _reads_with_exceptions()
    lib = fake_caller_lib()
    nc = F.NativeCaller(0, 1, 1, lib=lib)
    try:
        for _ in range(2):
            with pytest.raises(_lib.PlatypusDeviceError) as e:
                nc.call_fetched_regions([F.FetchedRegion.from_reads("20", 100, 300, fasta, [(reads, [])], packed=True)], ["S1"], default_options())
            assert e.value.code == -6 and "plat_read_buffers" in str(e.value)
        assert nc.call_regions([], ["S1"], default_options()) == ""
    finally:
        nc.close()


def test_fake_engine_binds_without_the_packed_entry_point():
    from tests.fakedev import fake_engine
    eng = fake_engine()
    assert not hasattr(eng.lib, "plat_read_buffers_packed_batch") or eng.lib.plat_read_buffers_packed_batch.argtypes
    assert eng.lib.plat_read_qc_batch.argtypes
