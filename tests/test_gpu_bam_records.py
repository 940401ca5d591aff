"""GPU tests of raw BAM alignment records as input: plat_bam_decode_batch (ReadIterator.get, htslibWrapper.pyx:328-406, on the device)
field for field against the reads the reference's loader was handed (tests/golden/region_fetched_cases.json.gz) and against hand-written
edge records, and plat_call_bam_regions against plat_call_fetched_regions on ASCII tables of the same reads.

A BAM record holds no `end`: the decoder derives it (bam_endpos of an htslib 1.x before 1.10: pos + 1 for an unmapped record or one without
a CIGAR, else pos + the reference length of the CIGAR, which may be 0 -- from the record's own pos, not the soft-clip-adjusted one).  The
expected `end` here is that rule, never what the code under test gave."""
import copy
import gzip
import json
import os
import struct

import numpy as np
import pytest

from platypus_amd import _lib, fastcaller as F, hostapi as H, synth
from platypus_amd.options import default_options

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
LETTERS = "=ACMGRSVTWYHKDBN"


def _cases():
    with gzip.open(os.path.join(HERE, "golden", "region_fetched_cases.json.gz"), "rt") as f:
        return json.load(f)


def _lead_clip(cigar):
    return cigar[0][1] if cigar and cigar[0][0] == 4 else 0


def _rule_end(pos, flag, cigar):
    """bam_endpos as the decode rules state it; `pos` is the read's (soft-clip-adjusted) position."""
    rec_pos = pos + _lead_clip(cigar)
    if (flag & 4) or not cigar:
        return rec_pos + 1
    return rec_pos + sum(ln for op, ln in cigar if op in (0, 2, 3, 7, 8))


def _aligned(x, end=None):
    return H.AlignedRead(x["seq"].encode(), bytes(ord(c) - 33 for c in x["qual"]), x["pos"], x["mapq"], x["flag"],
                         end=x["end"] if end is None else end, cigarOps=[tuple(c) for c in x["cigar"]], chromID=x.get("chromID", 0),
                         mateChromID=x.get("mateChromID", 0), insertSize=x.get("insertSize", 0), matePos=x["matePos"])


def test_decode_matches_the_fixture_reads_field_for_field():
    """Every read of the 41 fetched cases (fetched and broken mates, 23 403 reads) encoded as a record and decoded on the device: bases,
    qualities, CIGAR pairs, pos, mapq, flags, chromID, mateChromID, insertSize and matePos are the fixture's; end is the rule's.  The
    fixture's stand-in loader wrote end = pos + reference length for the 901 reads with a leading soft clip (get gives pos + clip +
    reference length), and two reads (cases 2 and 6) carry an end unrelated to their CIGAR: 903 of 23 403 differ from the rule, asserted
    so that a fixture change is noticed.  The records lie at odd offsets, with names of 1-255 bytes, aux data behind them, block_size
    words between them, in an order other than rec_off's."""
    reads = [x for c in _cases() for r in c["regions"] for s in r["samples"] for key in ("fetched", "brokenMates") for x in s[key]]
    n = len(reads)
    assert n == 23403
    # every fixture read is encodable
    assert all(set(x["seq"]) <= set(LETTERS) and len(x["seq"]) > 0 for x in reads)
    assert max(ord(c) - 33 for x in reads for c in x["qual"]) <= 93
    assert {op for x in reads for op, _ in x["cigar"]} <= {0, 1, 2, 4}
    assert max(len(x["cigar"]) for x in reads) <= 6 and max(ln for x in reads for _, ln in x["cigar"]) <= 150
    assert min(x["pos"] + _lead_clip(x["cigar"]) for x in reads) >= 0
    rule_end = [_rule_end(x["pos"], x["flag"], x["cigar"]) for x in reads]
    differs = [i for i, x in enumerate(reads) if rule_end[i] != x["end"]]
    assert len(differs) == 903 and sum(1 for x in reads if _lead_clip(x["cigar"])) == 901
    assert sum(1 for i in differs if _lead_clip(reads[i]["cigar"])) == 901
    # the blob: records in a shuffled order, each behind a block_size word and a gap of 0-3 bytes, names and aux data of many lengths
    rng = np.random.default_rng(20)
    recs = []
    for i, x in enumerate(reads):
        name = bytes(rng.integers(33, 127, size=(0, 1, 17, 40, 254)[i % 5], dtype=np.uint8)) + b"\0"
        aux = bytes(rng.integers(0, 256, size=int(rng.integers(0, 30)), dtype=np.uint8))
        recs.append(synth.bam_record(_aligned(x), name, aux))
    assert {len(r[32:32 + r[8]]) for r in recs} >= {1, 2, 255}
    parts, off, at = [b"\x5a"], np.zeros(n, dtype=np.int64), 1
    for i in rng.permutation(n):
        gap = int(rng.integers(0, 4))
        parts.append(b"\xa5" * gap + struct.pack("<i", len(recs[i])))
        at += gap + 4
        off[i] = at
        parts.append(recs[i])
        at += len(recs[i])
    blob = np.frombuffer(b"".join(parts), dtype=np.uint8)
    assert len({int(o) & 3 for o in off}) == 4 and not np.all(np.diff(off) > 0)
    got = H.get_engine().bam_decode(blob, off)
    assert list(got["status"]) == [0, -1, sum(len(x["seq"]) for x in reads), sum(len(x["cigar"]) for x in reads)] and got["guard_intact"]
    assert list(np.diff(got["off"])) == [len(x["seq"]) for x in reads] and got["off"][0] == 0
    assert list(np.diff(got["cig_off"])) == [len(x["cigar"]) for x in reads] and got["cig_off"][0] == 0
    assert got["seq"].tobytes() == "".join(x["seq"] for x in reads).encode()
    assert got["qual"].tobytes() == b"".join(bytes(ord(c) - 33 for c in x["qual"]) for x in reads)
    assert got["cigar"].tolist() == [list(c) for x in reads for c in x["cigar"]]
    for key, name in (("pos", "pos"), ("mapq", "mapq"), ("flags", "flag"), ("chrom_id", "chromID"), ("mate_chrom_id", "mateChromID"),
                      ("insert_size", "insertSize"), ("mate_pos", "matePos")):
        assert got[key].tolist() == [x[name] for x in reads], key
    assert got["end"].tolist() == rule_end


def _rec(ref_id=0, pos=1000, name=b"r\0", mapq=60, cigar=((0, 10),), flag=3, codes=(1, 2, 4, 8, 1, 2, 4, 8, 1, 2), qual=None, next_ref=0,
         next_pos=1200, tlen=250, aux=b"", l_seq=None, n_cigar=None):
    """A record written field by field (SAM/BAM specification 4.2, from refID on); l_seq / n_cigar override what the arrays say."""
    codes = list(codes)
    qual = bytes(qual if qual is not None else [30] * len(codes))
    packed = codes + [0] * (len(codes) & 1)
    return (struct.pack("<iiBBHHHiiii", ref_id, pos, len(name), mapq, 0, len(cigar) if n_cigar is None else n_cigar, flag,
                        len(codes) if l_seq is None else l_seq, next_ref, next_pos, tlen) + name +
            b"".join(struct.pack("<I", (ln << 4) | op) for op, ln in cigar) +
            bytes((packed[i] << 4) | packed[i + 1] for i in range(0, len(packed), 2)) + qual + aux)


def _blob(recs, lead=1):
    off, at = [], lead
    for r in recs:
        off.append(at)
        at += len(r)
    return np.frombuffer(b"\x00" * lead + b"".join(recs), dtype=np.uint8), np.array(off, dtype=np.int64)


def test_edge_records_decode_by_the_rule():
    eng = H.get_engine()
    rng = np.random.default_rng(7)
    lens = [1, 2, 15, 16, 17, 31, 32, 33, 150, 251]
    recs, want = [], []

    def add(rec, seq, qual, cig, pos, end, **f):
        recs.append(rec)
        want.append(dict(dict(seq=seq, qual=list(qual), cigar=[list(c) for c in cig], pos=pos, end=end, mapq=60, flags=3, chrom_id=0,
                              mate_chrom_id=0, insert_size=250, mate_pos=1200), **f))
    # all 16 base codes
    add(_rec(codes=range(16), cigar=[(0, 16)]), LETTERS, [30] * 16, [(0, 16)], 1000, 1016)
    # lengths around the 16-base step, qualities 0 / 93 / 254 among them (a quality above 93 is passed through as the byte it is)
    for n in lens:
        codes = rng.integers(0, 16, size=n).tolist()
        q = rng.choice([0, 1, 20, 40, 93, 94, 200, 254], size=n).tolist()
        q[0] = (0, 93, 254)[n % 3]
        add(_rec(codes=codes, qual=q, cigar=[(0, n)], name=bytes(rng.integers(65, 91, size=n % 7, dtype=np.uint8)) + b"\0"),
            "".join(LETTERS[c] for c in codes), q, [(0, n)], 1000, 1000 + n)
    # every CIGAR op: M D N = X count towards end
    every = [(0, 3), (1, 2), (2, 4), (3, 5), (4, 1), (5, 2), (6, 3), (7, 4), (8, 5)]
    add(_rec(cigar=every), "ACGTACGTAC", [30] * 10, every, 1000, 1000 + 3 + 4 + 5 + 4 + 5)
    # a leading S moves pos, end counts from the record's own pos
    add(_rec(cigar=[(4, 7), (0, 3)]), "ACGTACGTAC", [30] * 10, [(4, 7), (0, 3)], 993, 1003)
    # a leading H followed by S does not
    add(_rec(cigar=[(5, 3), (4, 7), (0, 3)]), "ACGTACGTAC", [30] * 10, [(5, 3), (4, 7), (0, 3)], 1000, 1003)
    # THE PINNED CASE: mapped, a CIGAR that consumes no reference (only S and I): end == the record's pos (htslib before 1.10; pos + 1 later)
    add(_rec(cigar=[(4, 5), (1, 5)]), "ACGTACGTAC", [30] * 10, [(4, 5), (1, 5)], 995, 1000)
    # no CIGAR: pos + 1
    add(_rec(cigar=[]), "ACGTACGTAC", [30] * 10, [], 1000, 1001)
    # unmapped with a CIGAR: pos + 1
    add(_rec(flag=4 | 1), "ACGTACGTAC", [30] * 10, [(0, 10)], 1000, 1001, flags=5)
    # negative refID / next_refID / next_pos, a negative tlen, the largest values a short holds
    add(_rec(ref_id=-1, pos=-1, next_ref=-1, next_pos=-1, tlen=-7, flag=4, mapq=255, cigar=[]), "ACGTACGTAC", [30] * 10, [], -1, 0,
        chrom_id=-1, mate_chrom_id=-1, mate_pos=-1, insert_size=-7, flags=4, mapq=255)
    add(_rec(ref_id=32767, next_ref=32767, cigar=[(0, 32767)], flag=65535 & ~4), "ACGTACGTAC", [30] * 10, [(0, 32767)], 1000, 1000 + 32767,
        chrom_id=32767, mate_chrom_id=32767, flags=65535 & ~4)
    # an odd length whose last nibble is the blob's last byte but for its qualities: the record ends where the blob ends
    codes = rng.integers(0, 16, size=33).tolist()
    add(_rec(codes=codes, cigar=[(0, 33)]), "".join(LETTERS[c] for c in codes), [30] * 33, [(0, 33)], 1000, 1033)
    for lead in (0, 1, 2, 3):
        blob, off = _blob(recs, lead)
        assert int(off[-1]) + len(recs[-1]) == len(blob)
        got = eng.bam_decode(blob, off)
        assert got["guard_intact"] and int(got["status"][0]) == 0
        for i, w in enumerate(want):
            a, b, c0, c1 = got["off"][i], got["off"][i + 1], got["cig_off"][i], got["cig_off"][i + 1]
            assert got["seq"][a:b].tobytes().decode() == w["seq"], (lead, i)
            assert got["qual"][a:b].tolist() == w["qual"], (lead, i)
            assert got["cigar"][c0:c1].tolist() == w["cigar"], (lead, i)
            for k in ("pos", "end", "mapq", "flags", "chrom_id", "mate_chrom_id", "insert_size", "mate_pos"):
                assert int(got[k][i]) == w[k], (lead, i, k)
    # an empty batch
    got = eng.bam_decode(np.zeros(0, np.uint8), np.zeros(0, np.int64))
    assert list(got["status"]) == [0, -1, 0, 0] and got["guard_intact"] and list(got["off"]) == [0]


def test_refused_records_name_the_record_and_leave_the_engine_usable():
    eng = H.get_engine()
    good = [_rec(), _rec(cigar=[(4, 2), (0, 8)]), _rec(codes=range(16), cigar=[(0, 16)])]
    big = list(range(16)) * 2048                                     # 32768 bases
    bad = {
        "l_seq 0": _rec(l_seq=0),
        "l_seq < 0": _rec(l_seq=-5),
        "qual[0] == 0xff": _rec(qual=[255] + [30] * 9),
        "l_seq 32768": _rec(codes=big, cigar=[(0, 100)]),
        "cigar length 32768": _rec(cigar=[(0, 32768)]),
        "refID 32768": _rec(ref_id=32768),
        "next_refID 40000": _rec(next_ref=40000),
        "n_cigar_op 32768": _rec(cigar=[(0, 1)] * 32768, codes=[1] * 10),
        "cigar op 9": _rec(cigar=[(0, 5), (9, 5)]),
        "pos under int32 after the soft clip": _rec(pos=-2147483648 + 3, cigar=[(4, 10)]),
    }

    def check_good(got, recs, skip=None):
        for i, r in enumerate(recs):
            if i == skip:
                assert got["off"][i + 1] == got["off"][i] and got["cig_off"][i + 1] == got["cig_off"][i]
                continue
            l_seq = struct.unpack_from("<i", r, 16)[0]
            assert got["off"][i + 1] - got["off"][i] == l_seq
            seq_at = 32 + r[8] + 4 * struct.unpack_from("<H", r, 12)[0]
            codes = [(r[seq_at + j // 2] >> (0 if j & 1 else 4)) & 15 for j in range(l_seq)]
            assert got["seq"][got["off"][i]:got["off"][i + 1]].tobytes().decode() == "".join(LETTERS[c] for c in codes)
            assert got["qual"][got["off"][i]:got["off"][i + 1]].tobytes() == r[seq_at + (l_seq + 1) // 2:seq_at + (l_seq + 1) // 2 + l_seq]

    for why, rec in bad.items():
        for at in (0, 2, 3):
            recs = good[:at] + [rec] + good[at:]
            blob, off = _blob(recs, 3)
            got = eng.bam_decode(blob, off, check=False)
            assert int(got["status"][0]) == -9 and int(got["status"][1]) == at, (why, at, got["status"])
            assert got["guard_intact"], why
            check_good(got, recs, skip=at)                           # the kernel carried on: the other records are decoded
            with pytest.raises(_lib.PlatypusDeviceError) as e:
                eng.bam_decode(blob, off)
            assert e.value.code == -9 and ("record %d" % at) in str(e.value)
        blob, off = _blob(good)
        check_good(eng.bam_decode(blob, off), good)                  # ... and the context is usable
    # a record that runs past the blob: its last byte cut off; an offset outside the blob; a record past its own limit
    blob, off = _blob(good, 2)
    got = eng.bam_decode(blob[:-1], off, check=False)
    assert list(got["status"][:2]) == [-9, 2] and got["guard_intact"]
    for o in (-1, len(blob) - 31, len(blob) + 100):
        got = eng.bam_decode(blob, np.array([off[0], o, off[2]]), check=False)
        assert list(got["status"][:2]) == [-9, 1] and got["guard_intact"]
    got = eng.bam_decode(blob, off, rec_limit=[len(blob), off[2] - 1, len(blob)], check=False)
    assert list(got["status"][:2]) == [-9, 1]
    check_good(eng.bam_decode(blob, off, rec_limit=[off[1], off[2], len(blob)]), good)
    # two bad records: the first is named
    recs = [good[0], bad["cigar op 9"], good[1], bad["l_seq 0"]]
    got = eng.bam_decode(*_blob(recs), check=False)
    assert list(got["status"][:2]) == [-9, 1]
    # capacities: one base or one pair short is PLAT_ERR_OVERFLOW at the record that does not fit, and nothing is written
    blob, off = _blob(good)
    bases, pairs = 10 + 10 + 16, 1 + 2 + 1
    for kw, who in ((dict(cap_bases=bases - 1, cap_pairs=pairs), 2), (dict(cap_bases=bases, cap_pairs=pairs - 1), 2), (dict(cap_bases=15, cap_pairs=pairs), 1),
                    (dict(cap_bases=0, cap_pairs=0), 0)):
        got = eng.bam_decode(blob, off, check=False, **kw)
        assert list(got["status"]) == [-8, who, bases, pairs] and got["guard_intact"], kw
        with pytest.raises(_lib.PlatypusDeviceError) as e:
            eng.bam_decode(blob, off, **kw)
        assert e.value.code == -8
    got = eng.bam_decode(blob, off, cap_bases=bases, cap_pairs=pairs)
    assert list(got["status"]) == [0, -1, bases, pairs] and got["guard_intact"]
    check_good(got, good)


def _fetched_and_bam(case, after):
    """The regions of one case for both calls: ASCII tables with end by the rule, and records."""
    from tests.region_golden import _reads
    fasta = H.FastaFile({"20": case["ref"].encode()})
    fetched, bam = [], []
    for r, rr in zip(case["regions"], after["regions"]):
        samples = []
        for i, s in enumerate(r["samples"]):
            fr = [_aligned(x, _rule_end(x["pos"], x["flag"], x["cigar"])) for x in s["fetched"]]
            br = _reads(rr["samples"][i]["brokenMates"]) if rr["loaded"] else []
            for b in br:
                b.end = _rule_end(b.pos, b.bitFlag, b.cigarOps)
            samples.append((fr, br))
        fetched.append(F.FetchedRegion.from_reads(r["chrom"], r["start"], r["end"], fasta, samples))
        bam.append(F.BamRegion.from_reads(r["chrom"], r["start"], r["end"], fasta, samples, lead=1, block_size=True))
    return fetched, bam


def test_bam_region_loop_equals_the_fetched_loop_on_all_cases():
    """All 41 cases through plat_call_bam_regions: text, rlen, skipped regions, per-sample counts and region text lengths are those of
    plat_call_fetched_regions on ASCII tables of the same reads with end set by the rule (tests/test_gpu_fetched_reads.py pins that path to
    the reference's 245 lines).  Printed, not asserted: how many cases also give the committed reference lines verbatim."""
    cases = _cases()
    with gzip.open(os.path.join(HERE, "golden", "region_cases.json.gz"), "rt") as f:
        after = json.load(f)
    assert len(cases) == 41
    nc = F.NativeCaller(0, 2, 2)
    verbatim = n_lines = n_skipped = 0
    try:
        for ci, (case, ref) in enumerate(zip(cases, after)):
            fetched, bam = _fetched_and_bam(case, ref)
            o1, o2 = default_options(**case["options"]), default_options(**case["options"])
            want = nc.call_fetched_regions(fetched, case["sample_names"], o1)
            want_loaded, want_counts, want_lens = list(nc.loaded), nc.read_counts.copy(), nc.region_text_lengths(len(fetched)).copy()
            got = nc.call_bam_regions(bam, case["sample_names"], o2)
            assert got == want, ci
            assert o2.rlen == o1.rlen, ci
            assert nc.loaded == want_loaded == [int(r["loaded"]) for r in case["regions"]], ci
            assert np.array_equal(nc.read_counts, want_counts), ci
            assert np.array_equal(nc.region_text_lengths(len(bam)), want_lens), ci
            assert nc.stats["input_bytes"] == sum(len(d) for k, reg in enumerate(bam) if want_loaded[k] for pair in reg.samples for d, o in pair if len(o))
            verbatim += got.split("\n")[:-1] == case["lines"]
            n_lines += got.count("\n")
            n_skipped += want_loaded.count(0)
    finally:
        nc.close()
    print("cases that give the committed reference lines verbatim with the rule's end: %d of %d (%d lines)" % (verbatim, len(cases), n_lines))
    assert n_skipped >= 1 and n_lines > 200


def _rule_ends(reads):
    out = copy.deepcopy(reads)
    for r in out:
        r.end = _rule_end(r.pos, r.bitFlag, r.cigarOps)
    return out


def test_synthetic_regions_equal_the_ascii_fetched_call():
    """Nine synthetic config-4 regions with the loader's trouble injected (duplicates, unmapped reads and mates, soft clips, ...), 1-3
    samples: the same text, counts and rlen as the ASCII fetched call on the same reads (end by the rule: a record holds none)."""
    groups = {1: [], 2: [], 3: []}
    for idx, nS in ((0, 1), (1, 2), (2, 1), (3, 3), (4, 2), (5, 1), (6, 3), (7, 2), (8, 1)):
        reg, samples = synth.config4_fetched_region(idx, region_len=20000, n_samples=nS)
        samples = [_rule_ends(rs) for rs in samples]
        fasta = H.FastaFile({reg["chrom"]: reg["ref"].tobytes()})
        pairs = [(rs, []) for rs in samples]
        groups[nS].append((F.FetchedRegion.from_reads(reg["chrom"], reg["start"], reg["end"], fasta, pairs),
                           F.BamRegion.from_reads(reg["chrom"], reg["start"], reg["end"], fasta, pairs, lead=3)))
    assert sum(len(g) for g in groups.values()) >= 8
    nc = F.NativeCaller(0, 2, 2)
    try:
        for nS, regs in groups.items():
            nm = ["S%d" % (i + 1) for i in range(nS)]
            o1, o2 = default_options(), default_options()
            want = nc.call_fetched_regions([f for f, _ in regs], nm, o1)
            counts = nc.read_counts.copy()
            got = nc.call_bam_regions([b for _, b in regs], nm, o2)
            assert got == want and o1.rlen == o2.rlen and np.array_equal(nc.read_counts, counts)
            assert want.count("\n") > 5 and 0 < counts[:, :, 1].sum() < counts[:, :, 0].sum()
    finally:
        nc.close()


def test_unsorted_and_bad_records_are_refused_and_the_caller_stays_usable():
    ref = b"ACGTTGCA" * 100
    fasta = H.FastaFile({"20": ref})

    def reads(order):
        return [H.AlignedRead(ref[p:p + 60], bytes([30] * 60), p, bitFlag=3) for p in order]

    def region(order):
        return F.BamRegion.from_reads("20", 100, 500, fasta, [(reads(order), [])])
    nc = F.NativeCaller(0, 1, 2)
    try:
        with pytest.raises(_lib.PlatypusDeviceError) as e:
            nc.call_bam_regions([region([100, 140, 180]), region([200, 150, 250])], ["S1"], default_options())
        assert e.value.code == -9 and "region 1" in str(e.value)
        assert "are not sorted by position (a BAM fetch is coordinate-sorted; the reference would sort them with an unstable qsort)" in str(e.value)
        nc.call_bam_regions([region([100, 140, 180, 200, 220])], ["S1"], default_options())
        assert nc.loaded == [1] and list(nc.read_counts[0][0][:2]) == [5, 0]
        # a record that cannot be decoded: the message names region, sample and record
        data, off = synth.bam_records(reads([100, 140, 180]))
        data = data.copy()
        struct.pack_into("<i", data, int(off[1]) + 16, 0)               # l_seq = 0
        broken = F.BamRegion("20", 100, 500, ref, [((data, off), (np.zeros(0, np.uint8), np.zeros(0, np.int64)))])
        with pytest.raises(_lib.PlatypusDeviceError) as e:
            nc.call_bam_regions([region([100, 140]), broken], ["S1"], default_options())
        assert e.value.code == -9 and "region 1" in str(e.value) and "sample 0" in str(e.value) and "record 1" in str(e.value)
        # a record listed twice outgrows the bound the blob's length gives
        twice = F.BamRegion("20", 100, 500, ref, [((data[:int(off[1])], np.array([off[0]] * 3)), (np.zeros(0, np.uint8), np.zeros(0, np.int64)))])
        with pytest.raises(_lib.PlatypusDeviceError) as e:
            nc.call_bam_regions([twice], ["S1"], default_options())
        assert e.value.code == -8 and "region 0" in str(e.value)
        want = nc.call_fetched_regions([F.FetchedRegion.from_reads("20", 100, 500, fasta, [(reads([100, 140, 180, 200, 220]), [])])], ["S1"], default_options())
        assert nc.call_bam_regions([region([100, 140, 180, 200, 220])], ["S1"], default_options()) == want
    finally:
        nc.close()
