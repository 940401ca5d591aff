"""GPU test of the refusals that the whole-file entry points (include/platypus_caller_bamfile.h) hand on from the device batch behind them
-- the upload, the inflate and the record walk of plat_call_bam_files, plat_bam_files_mates_plan and plat_call_bam_files_mates -- with
their messages in full, the region, file, sample, query and chunk in them included.  The strings were taken from the library before the
two batches shared their code; the virtual offsets in them are read off the file's own index.  Every refusal is a status the device
writes or a check the host makes before anything is uploaded: an error return of the library, none provokes a fault.

One file (tests/bam_file_cases.py) of 27 records of 40 bases on an 80 kb contig, in blocks of 120 bytes: 8 in region 0, 8 in region 1, 3
of them improper pairs, 8 further on and then the 3 mates, every group in a 16 kb window of its own, so that a fetch's chunks end where
its own records end."""
import struct

import numpy as np
import pytest

from platypus_amd import _lib, fastcaller as F, tabixindex
from platypus_amd.options import default_options
from tests import bam_file_cases as B
from tests.test_gpu_bam_mates import BOTH, _read

pytestmark = pytest.mark.gpu

REFS = [("chrA", 80000), ("chrB", 30000)]
REGIONS = [("chrA", 1000, 2000), ("chrA", 20000, 21000)]
WHERE = ["region %d (%s:%d-%d)" % ((k,) + r) for k, r in enumerate(REGIONS)]
MATES_AT, QUERY = 60000, "query 0 (chrA:60000-60101)"
WALK_FAILS = " fails (a block_size below 32, or a record or its CIGAR running past the chunk's bytes)"
NO_INFLATE = " cannot be inflated (a bad header, an invalid deflate stream, output other than ISIZE bytes, or a CRC32 mismatch)"
CONTIG = bytes(b"ACGT"[int(v)] for v in np.random.default_rng(5).integers(0, 4, REFS[0][1]))


def records(merged):
    """[record]; the improper pairs are records 10, 12 and 14, their mates the last three."""
    rg = (lambda i: (b"g1", b"g2")[i % 2]) if merged else (lambda i: None)
    out = []
    for base in (1050, 20050, 40050):
        for i in range(8):
            p = base + 100 * i
            improper = base == 20050 and i in (2, 4, 6)
            flag, mpos = (0x41, MATES_AT + 25 * (i - 2)) if improper else (0x43, p + 200)
            out.append(_read(0, p, flag, 0, mpos, CONTIG[p:p + 40], b"r%d\0" % len(out), rg(len(out))))
    for j in range(3):
        p = MATES_AT + 50 * j
        out.append(_read(0, p, 0x81, 0, 20250 + 200 * j, CONTIG[p:p + 40], b"m%d\0" % j, rg(j)))
    return out


def built(merged, recs=None):
    rgs = [("g1", "S1"), ("g2", "S2")] if merged else [("g1", "S1")]
    text = "@HD\tVN:1.4\tSO:coordinate\n" + B.sq_lines(REFS) + "".join("@RG\tID:%s\tSM:%s\n" % g for g in rgs)
    return B.built(dict(name="messages.bam", text=text, refs=REFS, records=recs or records(merged)))


def refused(call, code, entry, message):
    with pytest.raises(_lib.PlatypusDeviceError) as e:
        call()
    assert e.value.code == code and str(e.value) == str(_lib.PlatypusDeviceError(code, message, entry))


@pytest.mark.parametrize("merged", [False, True])
def test_a_block_size_of_31_in_region_1_is_refused_with_the_whole_message_by_every_entry_point(merged):
    """(a) the third record of region 1: region 0's walk ends in front of it."""
    recs = records(merged)
    recs[10] = struct.pack("<i", 31) + recs[10][4:]
    good, bad = built(merged), built(merged, recs)
    regions = [F.BamFilesRegion(c, s, e, CONTIG) for c, s, e in REGIONS]
    plain, both = default_options(), default_options(**BOTH)
    behind, unit = ("plat_call_bgzf_regions_rg", "file 0") if merged else ("plat_call_bgzf_regions", "sample 0")
    plan = "plat_bam_files_mates_plan"
    nc = F.NativeCaller(0, 1, 2)
    try:
        g, b = (nc.open_bam(f["bam"], f["bai"], f["name"]) for f in (good, bad))
        text = nc.call_bam_files([g], regions, plain)
        refused(lambda: nc.call_bam_files([b], regions, plain), -9, "plat_call_bam_files", behind + ": the record walk of " + WHERE[1] + ", " + unit + WALK_FAILS)
        assert nc.call_bam_files([g], regions, plain) == text and nc.loaded == [1, 1]
        refused(lambda: nc.bam_mates_plan([b], REGIONS, both), -9, plan, plan + ": the record walk of " + WHERE[1] + ", file 0" + WALK_FAILS)
        got = nc.bam_mates_plan([g], REGIONS, both)
        assert [len(u[0]["records"]) for u in got] == [0, 3] and got[1][0]["queries"] == [(0, MATES_AT, MATES_AT + 101)]
        with_mates = nc.call_bam_files_mates([g], regions, both)
        refused(lambda: nc.call_bam_files_mates([b], regions, both), -9, "plat_call_bam_files_mates", plan + ": the record walk of " + WHERE[1] + ", file 0" + WALK_FAILS)
        assert nc.call_bam_files_mates([g], regions, both) == with_mates and nc.loaded == [1, 1]
        g.close()
        b.close()
    finally:
        nc.close()


def test_round_two_names_the_chunk_it_cannot_cut_and_the_block_that_does_not_inflate():
    """(b) the file's bytes end in front of the block in which the first mate begins, (c) that block's CRC32 is off by its lowest bit: round
    one has every byte it asks for, round two refuses the query's one chunk."""
    f = built(False)
    at = f["placed"][-3][3] >> 16                                             # where the mates' block begins ...
    size = struct.unpack_from("<H", f["bam"], at + 16)[0] + 1                 # ... and its length
    chunks = tabixindex.BamIndex(f["bai"]).query(0, *B.window(MATES_AT, MATES_AT + 101))
    assert len(chunks) == 1 and chunks[0][0] >> 16 == at < chunks[0][1] >> 16
    for c, s, e in REGIONS:                                                   # round one's chunks end in front of that block
        first = tabixindex.BamIndex(f["bai"]).query(0, *B.window(s, e))
        assert first and all(v >> 16 < at for _, v in first) and B.first_chunk_off_the_data(f["bam"][:at], first) is None
    assert B.first_chunk_off_the_data(f["bam"][:at], chunks) == (0,) + chunks[0]
    flipped = f["bam"][:at + size - 8] + bytes([f["bam"][at + size - 8] ^ 1]) + f["bam"][at + size - 7:]
    regions = [F.BamFilesRegion(c, s, e, CONTIG) for c, s, e in REGIONS]
    both = default_options(**BOTH)
    plan = "plat_bam_files_mates_plan"
    place = WHERE[1] + ", file 0, " + QUERY
    nc = F.NativeCaller(0, 1, 2)
    try:
        g, cut, crc = (nc.open_bam(data, f["bai"], f["name"]) for data in (f["bam"], f["bam"][:at], flipped))
        text = nc.call_bam_files([g], regions, default_options())
        for h, message in ((cut, "chunk 0 of %s (virtual offsets %d .. %d) %s" % ((place,) + chunks[0] + (B.NO_CUT,))), (crc, "block 0 of " + place + ", chunk 0" + NO_INFLATE)):
            assert nc.call_bam_files([h], regions, default_options()) == text                 # round one's fetches alone
            refused(lambda: nc.bam_mates_plan([h], REGIONS, both), -9, plan, plan + ": " + message)
            refused(lambda: nc.call_bam_files_mates([h], regions, both), -9, "plat_call_bam_files_mates", plan + ": " + message)
            assert [len(u[0]["records"]) for u in nc.bam_mates_plan([g], REGIONS, both)] == [0, 3]
        for h in (g, cut, crc):
            h.close()
    finally:
        nc.close()
