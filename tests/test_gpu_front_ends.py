"""GPU tests of what the record front ends share: on ONE small region list the seven ways in (fetched tables ASCII and packed, raw BAM
records, BGZF blocks, merged files as records and as BGZF blocks in one and in two chunks) give the same text, rlen, loaded, per-sample
counts, region text lengths and stats, and every refusal that goes through a shared message path says exactly what this file formats
itself.  tests/test_gpu_fetched_reads.py pins the ASCII fetched path to the reference; the other test files compare the front ends on
the fixture's 41 cases and check the refusals by substring.

The list: contig "20" of 800 bases, two samples, three regions with 4+3, 6+5 and 4+3 fetched reads of 60 bases, a SNP in the reads of the
outer two, one broken mate in the last, maxReads = 11 -- the loader gives up on exactly the middle region.  Every refusal here is an
error return of the library; none provokes a fault."""
import struct
import zlib

import numpy as np
import pytest

from platypus_amd import _lib, fastcaller as F, hostapi as H, synth
from platypus_amd.options import default_options

pytestmark = pytest.mark.gpu

REF = b"ACGTTGCA" * 100
NAMES = ["S1", "S2"]
BOUNDS = [(100, 300), (300, 500), (500, 700)]
STARTS = [([100, 120, 140, 160], [110, 130, 150]), ([300, 320, 340, 360, 380, 400], [310, 330, 350, 370, 390]), ([500, 520, 540, 560], [510, 530, 550])]
SNPS = (165, 565)                                            # G -> T in every read that covers them (regions 0 and 2)
GROUPS = {"lane0a": 0, "lane0b": 0, "lane1": 1}
TABLE_BYTES = sum(len(g) for g in GROUPS) + 8 * len(GROUPS)
MAX_READS = 11
UNSORTED = ("are not sorted by position (a BAM fetch is coordinate-sorted; the reference would sort them with an unstable qsort)")
NO_DECODE = (" cannot be decoded (it runs past its blob, has no bases or no qualities, a CIGAR operation above 8, or a length, reference id or "
             "position the reference's read would not hold)")
NO_INFLATE = " cannot be inflated (a bad header, an invalid deflate stream, output other than ISIZE bytes, or a CRC32 mismatch)"


def _read(p, **kw):
    seq = bytearray(REF[p:p + 60])
    for s in SNPS:
        if p <= s < p + 60:
            assert seq[s - p:s - p + 1] == b"G"
            seq[s - p:s - p + 1] = b"T"
    return H.AlignedRead(bytes(seq), bytes([30] * 60), p, bitFlag=3, **kw)


def _lists(starts=STARTS, broken=((2, 1),)):
    """Per region, per sample (fetched, brokenMates); broken: the (region, sample) that hold one broken mate."""
    return [[([_read(p) for p in ps], [_read(a + 100, matePos=a + 80)] if (k, i) in broken else []) for i, ps in enumerate(per)]
            for k, ((a, _), per) in enumerate(zip(BOUNDS, starts))]


def _files(samples):
    """A region's samples as two merged files: sample 0 split over both in position order, sample 1 in file 0."""
    (f0, b0), (f1, b1) = samples
    h = len(f0) // 2
    return [[(0, "lane0a", f0[:h], b0), (1, "lane1", f1, b1)], [(0, "lane0b", f0[h:], [])]]


def _fasta():
    return H.FastaFile({"20": REF})


def _build(make, lists, **kw):
    return [make("20", a, b, _fasta(), samples, **kw) for (a, b), samples in zip(BOUNDS, lists)]


def _rg_build(make, lists, **kw):
    return [make("20", a, b, _fasta(), _files(samples), **kw) for (a, b), samples in zip(BOUNDS, lists)]


def _bytes_of(t):
    return sum(len(x[0]) for x in t)


# name -> (entry point, regions of a list, the call, the input bytes of a built region)
WAYS = {
    "ascii": ("plat_call_fetched_regions", lambda ls, **kw: _build(F.FetchedRegion.from_reads, ls), lambda nc, r, o, **kw: nc.call_fetched_regions(r, NAMES, o, **kw),
              lambda r: 2 * sum(int(t.off[t.n]) for s in r.samples for t in s[:2])),
    "packed": ("plat_call_fetched_regions", lambda ls, **kw: _build(F.FetchedRegion.from_reads, ls, packed=True), lambda nc, r, o, **kw: nc.call_fetched_regions(r, NAMES, o, **kw),
               lambda r: sum(int(t.off[t.n]) + 10 * len(t.exc[0]) for s in r.samples for t in s[:2])),
    "bam": ("plat_call_bam_regions", lambda ls, **kw: _build(F.BamRegion.from_reads, ls), lambda nc, r, o, **kw: nc.call_bam_regions(r, NAMES, o, **kw),
            lambda r: sum(_bytes_of(s) for s in r.samples)),
    "bgzf": ("plat_call_bgzf_regions", lambda ls, **kw: _build(F.BgzfRegion.from_reads, ls, **kw), lambda nc, r, o: nc.call_bgzf_regions(r, NAMES, o),
             lambda r: r.compressed_bytes + sum(len(b[0]) for _, b in r.samples)),
    "bam_rg": ("plat_call_bam_regions_rg", lambda ls, **kw: _rg_build(F.BamFileRegion.from_reads, ls), lambda nc, r, o: nc.call_bam_regions_rg(r, GROUPS, NAMES, o),
               lambda r: r.record_bytes),
    "bgzf_rg": ("plat_call_bgzf_regions_rg", lambda ls, **kw: _rg_build(F.BgzfFileRegion.from_reads, ls, **kw), lambda nc, r, o: nc.call_bgzf_regions_rg(r, GROUPS, NAMES, o),
                lambda r: r.compressed_bytes + sum(len(b[0]) for _, b in r.files)),
}
RECORD_WAYS = ("bam", "bgzf", "bam_rg", "bgzf_rg")


def _where(k, unit, i):
    return "region %d (20:%d-%d), %s %d" % (k, BOUNDS[k][0], BOUNDS[k][1], unit, i)


@pytest.fixture(scope="module")
def nc():
    caller = F.NativeCaller(0, 1, 2)                         # one worker, two regions per chunk
    yield caller
    caller.close()


@pytest.fixture(scope="module")
def base(nc):
    """The baseline: the ASCII fetched call on the list."""
    text = WAYS["ascii"][2](nc, WAYS["ascii"][1](_lists()), default_options(maxReads=MAX_READS))
    assert nc.loaded == [1, 0, 1]
    lines = text.split("\n")[:-1]
    assert any(ln.split("\t")[1] == str(SNPS[0] + 1) for ln in lines) and any(ln.split("\t")[1] == str(SNPS[1] + 1) for ln in lines), text
    return text


def _refused(nc, base, way, regions, code, message, good=None):
    """The call is refused with exactly `message`, and the same caller then gives the baseline text through the same entry point."""
    entry, build, call, _ = WAYS[way]
    with pytest.raises(_lib.PlatypusDeviceError) as e:
        call(nc, regions, default_options())
    assert e.value.code == code
    assert str(e.value) == str(_lib.PlatypusDeviceError(code, entry + ": " + message, entry))
    assert call(nc, build(_lists()) if good is None else good, default_options(maxReads=MAX_READS)) == base


def test_the_seven_ways_in_agree(nc, base):
    lists = _lists()
    assert [sum(len(f) for f, _ in s) for s in lists] == [7, MAX_READS, 7]
    got = {}
    for name, way, kw in [(w, w, {}) for w in ("ascii", "packed", "bam", "bgzf", "bam_rg")] + [("bgzf_rg/1", "bgzf_rg", dict(n_chunks=1)),
                                                                                              ("bgzf_rg/2", "bgzf_rg", dict(n_chunks=2))]:
        entry, build, call, input_bytes = WAYS[way]
        regions = build(lists, **kw)
        if kw:
            assert all(len(chunks) == kw["n_chunks"] for r in regions for chunks, _ in r.files)
        o = default_options(maxReads=MAX_READS)
        text = call(nc, regions, o)
        want_bytes = sum(input_bytes(r) for k, r in enumerate(regions) if k != 1) + (TABLE_BYTES if way.endswith("_rg") else 0)
        got[name] = (text, o.rlen, list(nc.loaded), nc.read_counts.tolist(), nc.region_text_lengths(3).tolist(), nc.stats["n_regions"])
        assert nc.stats["input_bytes"] == want_bytes, name
    first = got["ascii"]
    assert first[0] == base and first[2] == [1, 0, 1] and first[5] == 3
    assert first[4][1] == 0 and first[4][0] > 0 and first[4][2] > 0 and sum(first[4]) == len(base)
    assert [c[0] + c[1] for c in first[3][0]] == [4, 3] and first[3][1] == [[0] * 10] * 2 and [c[0] + c[1] for c in first[3][2]] == [4, 3]
    for name, g in got.items():
        assert g == first, name


def test_source_lines_stay_with_their_regions_and_go_with_the_call(nc, base):
    """Three lines, one per region, the middle one the dropped region's: both calls that take source lines give the text of the two loaded
    regions called alone with their own lines, another text than without lines, and the plain text again on the next call."""
    src = [b"20\t%d\t.\tG\tT\t50\tPASS\tAC=1\tGT\t0/1\n" % (p + 1) for p in (SNPS[0], 365, SNPS[1])]
    assert all(REF[p:p + 1] == b"G" for p in (SNPS[0], 365, SNPS[1]))
    texts = []
    for way in ("ascii", "bam"):
        _, build, call, _ = WAYS[way]
        texts.append(call(nc, build(_lists()), default_options(maxReads=MAX_READS), source_lines=src))
        assert nc.loaded == [1, 0, 1] and nc.stats["n_source_lines"] == 2 and nc.region_text_lengths(3)[1] == 0
        assert call(nc, build(_lists()), default_options(maxReads=MAX_READS)) == base
        assert nc.stats["n_source_lines"] == 0
    assert texts[0] == texts[1] and texts[0] != base and texts[0].count("\n") > 0
    _, build, call, _ = WAYS["ascii"]
    outer = build(_lists())
    assert call(nc, [outer[0], outer[2]], default_options(), source_lines=[src[0], src[2]]) == texts[0]


def test_an_unsorted_second_region_is_named_by_all_five_entry_points(nc, base):
    starts = [STARTS[0], ([300, 340, 320, 360, 380, 400], STARTS[1][1]), STARTS[2]]
    for way in ("ascii",) + RECORD_WAYS:
        _refused(nc, base, way, WAYS[way][1](_lists(starts)), -9, "the fetched reads of " + _where(1, "sample", 0) + " " + UNSORTED)


def test_a_broken_mate_record_past_its_blob_is_named(nc, base):
    """The one broken-mate record of region 0, sample 1, ten bytes short of its qualities."""
    lists = _lists(broken=((0, 1), (2, 1)))
    for way in ("bam", "bgzf"):
        regions = WAYS[way][1](lists)
        r = regions[0]
        first, (data, off) = r.samples[1]
        assert len(off) == 1
        cut = (first, (data[:-10], off))
        if way == "bam":
            regions[0] = F.BamRegion("20", 100, 300, REF, [r.samples[0], cut])
        else:
            regions[0] = F.BgzfRegion("20", 100, 300, REF, r.tid, r.itr_beg, r.itr_end, [r.samples[0], cut])
        _refused(nc, base, way, regions, -9, "broken-mate record 0 of " + _where(0, "sample", 1) + NO_DECODE)


def test_a_record_without_rg_is_named_with_its_file(nc, base):
    """Record 2 of file 0 of region 0 carries no RG field."""
    lists = _lists()
    entries = _files(lists[0])[0]
    reads, aux = F.merge_by_read_group([(s, g, rs) for s, g, rs, _ in entries], lambda r: r.pos)
    aux[2] = b""
    for way in ("bam_rg", "bgzf_rg"):
        regions = WAYS[way][1](lists)
        r = regions[0]
        if way == "bam_rg":
            data, off = synth.bam_records(reads, aux=aux)
            bare = (data, off, np.diff(np.append(off, len(data))).astype(np.int32))
            regions[0] = F.BamFileRegion("20", 100, 300, REF, [(bare, r.files[0][1]), r.files[1]])
        else:
            one = F.BgzfRegion.from_reads("20", 100, 300, _fasta(), [(reads, [])], aux=aux)
            regions[0] = F.BgzfFileRegion("20", 100, 300, REF, r.tid, r.itr_beg, r.itr_end, [(one.samples[0][0], r.files[0][1]), r.files[1]])
        _refused(nc, base, way, regions, -9, "fetched record 2 of " + _where(0, "file", 0) + " has no RG field")


def _edit_first_chunk(way, r, bounds, edit):
    """The region with the first chunk of its unit 0 (sample 0; file 0) replaced by edit(data, first_uoffset, end_coffset, end_uoffset)."""
    units = r.samples if way == "bgzf" else r.files
    chunks, broken = units[0]
    new = [([edit(*chunks[0])] + chunks[1:], broken)] + units[1:]
    return (F.BgzfRegion if way == "bgzf" else F.BgzfFileRegion)("20", bounds[0], bounds[1], REF, r.tid, r.itr_beg, r.itr_end, new)


def test_a_corrupted_block_is_named_with_its_unit(nc, base):
    """One flipped payload byte in the stored (level 0) block of region 2's first unit: the block inflates to its ISIZE bytes and the CRC32
    does not match -- the inflate reports it by status."""
    def flip(d, fu, ec, eu):
        d = bytearray(d.tobytes())
        bsize = struct.unpack_from("<H", d, 16)[0] + 1
        crc, isize = struct.unpack_from("<II", d, bsize - 8)
        assert zlib.crc32(zlib.decompress(bytes(d[18:bsize - 8]), -15)) == crc
        d[18 + 5 + 10] ^= 0x01                               # (18 header bytes, 5 of the stored block's own: a byte of the first record)
        out = zlib.decompress(bytes(d[18:bsize - 8]), -15)
        assert len(out) == isize and zlib.crc32(out) != crc
        return bytes(d), fu, ec, eu
    for way, unit in (("bgzf", "sample"), ("bgzf_rg", "file")):
        regions = WAYS[way][1](_lists(), level=0)
        regions[2] = _edit_first_chunk(way, regions[2], BOUNDS[2], flip)
        _refused(nc, base, way, regions, -9, "block 0 of " + _where(2, unit, 0) + ", chunk 0" + NO_INFLATE)


def test_blocks_that_do_not_chain_are_named_with_their_unit(nc, base):
    """Region 0's first unit in blocks of 200 bytes (three and the EOF block), the high byte of the second block's BSIZE flipped: the block
    then leaves its chunk's data, and the host's walk names the offset at which it starts."""
    at1 = []

    def flip(d, fu, ec, eu):
        d = bytearray(d.tobytes())
        at1.append(struct.unpack_from("<H", d, 16)[0] + 1)
        assert struct.unpack_from("<H", d, at1[-1] + 16)[0] < 32768 and len(d) < 32768 and d[at1[-1]:at1[-1] + 4] == b"\x1f\x8b\x08\x04"
        d[at1[-1] + 17] ^= 0x80
        return bytes(d), fu, ec, eu
    for way, unit in (("bgzf", "sample"), ("bgzf_rg", "file")):
        regions = WAYS[way][1](_lists(), block_payload=200)
        regions[0] = _edit_first_chunk(way, regions[0], BOUNDS[0], flip)
        _refused(nc, base, way, regions, -9, "the BGZF blocks of " + _where(0, unit, 0) + ", chunk 0 do not chain: no valid block header at offset %d of its data "
                 "(bad magic, no BC subfield, or a block that leaves the data)" % at1[-1])


def test_an_end_coffset_off_a_block_boundary_is_named_with_its_unit(nc, base):
    # "file" for plat_call_bgzf_regions_rg: the front-end refactor gives BgzfFront its unit word, so the host-side chunk checks of that call
    # say `file F` (they said `sample F` before, for a number that is a file index)
    for way, unit in (("bgzf", "sample"), ("bgzf_rg", "file")):
        regions = WAYS[way][1](_lists())
        regions[0] = _edit_first_chunk(way, regions[0], BOUNDS[0], lambda d, fu, ec, eu: (d, fu, 7, 0))
        _refused(nc, base, way, regions, -9, "end_coffset 7 of " + _where(0, unit, 0) + ", chunk 0 is not a block boundary of its data")
