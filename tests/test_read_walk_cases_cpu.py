"""The inputs of tests/test_gpu_read_walk_fuzz.py (tests/read_walk_cases.py) on the oracle alone: they must reach what they were written to
reach -- every CIGAR operation, records behind base 160 and 320 of a read, every alignment of the 2-bit words, read lists of three trips with
supporting reads in each -- or the comparisons on the device would hold without saying anything."""
import collections
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import read_walk_cases as C  # noqa: E402


@pytest.fixture(scope="module")
def scan():
    return C.scan_regions()


@pytest.fixture(scope="module")
def windows():
    return C.stats_windows()


def test_scan_reads_hold_every_length_operation_and_flavour(scan):
    regions, notes = scan
    reads = [r for g in regions for r in g["reads"]]
    assert set(C.LENGTHS) <= {len(r["seq"]) for r in reads}
    assert {op for r in reads for op, ln in r["cigar"]} == set(range(9))
    assert all(len(r["seq"]) == len(r["qual"]) == C.read_len(r["cigar"]) for r in reads)
    quals = np.frombuffer(b"".join(r["qual"] for r in reads), dtype=np.uint8)
    assert quals.max() <= 93 and (quals > 63).any()                                 # the reference asserts 0..93 (variant.pyx:564-565); > 63: packed exceptions
    for q in C.MIN_BASE_QUALS:
        assert {q - 1, q, q + 1} <= set(quals.tolist())
    bases = set(b"".join(r["seq"] for r in reads))
    assert bases == set(b"ACGTN")                                                   # what the scan on codes is promised
    names = collections.Counter(n for ns in notes for n in ns)
    for name in ("plain_a", "plain_b", "plain_c", "plain_late", "n_ends", "qcfail", "pairs", "clip", "h_x_n_eq_p", "m_i_m", "m_d_m", "i_first", "i_last",
                 "d_first", "d_last", "i_d", "d_i", "i_with_n", "d_over_n", "d_clamped", "d_clamped_away", "i_first_at_0"):
        assert names[name] >= 1, name
    for f in C.FLANKS:
        assert names["flank_%d_I" % f] >= 10 and names["flank_%d_D" % f] >= 10
    for g in regions:                                                               # every read inside its window (the clamped deletions end at its end)
        for r in g["reads"]:
            for op, ro, fp, ln in C.segments(r):
                assert g["ref_seq_start"] <= fp and fp + ln <= g["ref_seq_start"] + C.REF_LEN
    assert regions[1]["contig_len"] == regions[1]["ref_seq_start"] + C.REF_LEN
    assert any(b not in b"ACGTN" for b in regions[3]["ref"]) and all(all(b in b"ACGTN" for b in g["ref"]) for g in regions[:3])
    assert all(g["ref"].count(b"N") >= 12 for g in regions)


def test_scan_reads_lie_at_every_alignment_of_the_code_words(scan):
    regions, _ = scan
    for f in C.MIN_FLANKS:
        ra, fa = C.scan_alignments(regions, f)
        assert ra == set(range(32)) and fa == set(range(32))
    assert {g % 16 for g in C.source_gaps(64)} == set(range(1, 16))


def test_oracle_scan_reports_no_error_and_reaches_the_later_trips(scan, oracle):
    regions, notes = scan
    for f, q, gs, gi in C.SCAN_SETTINGS:
        n = snps = late = later = from_long = 0
        kinds = set()
        for g, ns in zip(regions, notes):
            rec = oracle.variant_candidates(g["ref"], g["ref_seq_start"], g["contig_len"], g["reads"], f, q, gs, gi)   # raises on -2: a read outside its window
            n += len(rec)
            for p, rem, add, ri in rec:
                from_long += len(g["reads"][ri]["seq"]) > 160
                kinds.add((bool(rem), bool(add)))
                assert not g["reads"][ri]["flag"] & 512                             # QCFail reads are skipped
                assert not (ns[ri] == "i_with_n" and not rem and len(add) == 3)     # an insertion that holds an N is dropped
                if rem and add:
                    i = C.read_index_of(g["reads"][ri], p)
                    snps += 1; late += i >= 160; later += i >= 320
        if gs:
            assert snps > 1500 and 4 * late >= snps and later > 100, (f, q, snps, late, later)
            assert 2 * from_long > n
        else:
            assert snps == 0
        assert ((False, True) in kinds and (True, False) in kinds and (False, False) in kinds) == bool(gi)    # insertions, deletions, and the deletion cut to nothing
    recs = oracle.variant_candidates(regions[0]["ref"], 0, regions[0]["contig_len"], regions[0]["reads"][:1], 3, 20)
    assert recs[0][0] == 0 and recs[0][1] == b"" and len(recs[0][2]) == 3           # the leading insertion at position 0: max(0, -1)


def test_the_flank_rule_and_the_pair_distances_decide_records(scan, oracle):
    """Indels between two M segments of f bases are reported exactly when f >= minFlank, and the mismatch pairs merge exactly when they are
    minFlank apart or less: the reads built for these rules meet them on the oracle."""
    regions, notes = scan
    for mf in C.MIN_FLANKS:
        seen = collections.Counter()
        for g, ns in zip(regions, notes):
            rec = oracle.variant_candidates(g["ref"], g["ref_seq_start"], g["contig_len"], g["reads"], mf, 20)
            indel = collections.Counter(ri for p, rem, add, ri in rec if bool(rem) != bool(add))
            for ri, name in enumerate(ns):
                if name and name.startswith("flank_") and name.endswith("_I"):
                    f = int(name.split("_")[1])
                    assert (indel[ri] == 1) == (f >= mf), (mf, name)
                    seen[f >= mf] += 1
        assert seen[True] and (seen[False] or mf == 0)
    g = C.Region(np.random.default_rng(1), 0, 10 ** 6)
    mism, quals, edit = C._pair_groups(200)
    g.read(100, [(C.M_, 200)], mism=mism, quals=quals, edit=edit)
    d = g.as_dict()
    spans = lambda mf: [(p - 100, len(rem)) for p, rem, add, ri in oracle.variant_candidates(d["ref"], 0, d["contig_len"], d["reads"], mf, 20)]
    assert (12, 1) in spans(0) and (13, 1) in spans(0) and (12, 2) in spans(3)
    assert (30, 4) in spans(3) and (50, 1) in spans(3) and (54, 1) in spans(3) and (50, 5) in spans(10)
    assert (75, 11) in spans(10) and (110, 1) in spans(10) and (121, 1) in spans(10)


def test_overflow_read_needs_more_than_its_slice(oracle):
    g = C.overflow_region()[0]
    per_read = collections.Counter(ri for p, rem, add, ri in oracle.variant_candidates(g["ref"], g["ref_seq_start"], g["contig_len"], g["reads"], 10, 20))
    assert per_read[1] > 40 and per_read[0] == 2 and per_read[2] == 2


def test_statistics_windows_hold_the_counts_and_shapes_asked_for(windows):
    goods, bads, ops, lens = set(), set(), set(), set()
    for n_ind, wins in windows.items():
        assert 1 <= n_ind <= 3
        for w in wins:
            assert len(w["samples"]) == n_ind and 1 <= len(w["variants"]) <= 8
            for s_ in w["samples"]:
                goods.add(len(s_["good"])); bads.add(len(s_["bad"]))
                for r in s_["good"] + s_["bad"]:
                    ops |= {op for op, ln in r["cigar"]}
                    lens.add(len(r["seq"]))
                    assert len(r["seq"]) == len(r["qual"]) == C.read_len(r["cigar"]) and max(r["qual"]) <= 93 and 0 <= r["mapq"] <= 60
            vig = np.array(w["var_in_genotype"])
            assert vig.shape == (len(w["variants"]), n_ind)
    assert goods == set(C.GOOD_COUNTS) and bads == set(C.BAD_COUNTS)
    assert ops == set(range(9)) and min(lens) == 1 and max(lens) >= 390
    variants = [v for wins in windows.values() for w in wins for v in w["variants"]]
    assert max(len(w["variants"]) for wins in windows.values() for w in wins) == 8
    ins, dele = {len(v["added"]) for v in variants if not v["removed"]}, {len(v["removed"]) for v in variants if not v["added"]}
    assert min(ins) == 1 and max(ins) >= 15 and min(dele) <= 3 and max(dele) >= 15
    assert any(len(v["removed"]) == len(v["added"]) == 1 for v in variants) and any(len(v["removed"]) == len(v["added"]) > 1 for v in variants)
    assert any(v["bam_min"] == v["bam_max"] == v["pos"] for v in variants) and any(v["bam_max"] - v["bam_min"] > 800 for v in variants)
    mixed = [np.array(w["var_in_genotype"]) for w in windows[3]]
    assert any((m.min(axis=1) != m.max(axis=1)).any() for m in mixed)               # in one sample's genotype and not in another's


def test_oracle_statistics_fill_every_column_and_every_trip(windows, oracle):
    total = np.zeros(16, dtype=np.int64)
    n_mmlq = three_trips = clamp_lo = clamp_hi = 0
    for n_ind, wins in windows.items():
        for w in wins:
            for brw, exact in C.STATS_SETTINGS:
                for counts, nr, nvr, mq in C.oracle_stats(oracle, w, brw, exact):
                    total += np.array(counts)
                    n_mmlq += len(mq)
                    assert len(mq) == counts[4] and sum(nr) == counts[0] and sum(nvr) == counts[2]
            for s, s_ in enumerate(w["samples"]):                                   # the sample's good reads 64 at a time, each trip as a sample of its own
                trips = [dict(good=s_["good"][k:k + 64], bad=[]) for k in range(0, len(s_["good"]), 64)]
                if len(trips) < 3:
                    continue
                res = oracle.variant_read_stats(w["variants"], trips, [[1] * len(trips)] * len(w["variants"]), 20, 11, 0)
                for v, (counts, nr, nvr, mq) in enumerate(res):
                    three_trips += w["var_in_genotype"][v][s] and sum(x > 0 for x in nvr) >= 3
            for v in w["variants"]:
                for s_ in w["samples"]:
                    for r in s_["good"]:
                        if r["pos"] <= v["bam_max"] and r["end"] > v["bam_min"]:
                            clamp_lo += v["bam_min"] - r["pos"] < 0
                            clamp_hi += v["bam_min"] - r["pos"] > len(r["seq"])
    assert (total > 0).all(), total.tolist()
    assert n_mmlq > 2000 and three_trips >= 5
    assert clamp_lo > 100 and clamp_hi > 0


def test_forced_supporters_straddle_the_lane_seams(windows, oracle):
    """Reads 62..65 and 126..129 (and 190..193) of a long good list support the first SNP, each with a window minimum of its own: a prefix that
    loses a trip's count, or lanes written out of order, changes the MMLQ list."""
    n = 0
    for wins in windows.values():
        for w in wins:
            for s, s_ in enumerate(w["samples"]):
                if len(s_["good"]) < 129:
                    continue
                assert w["var_in_genotype"][0][s] == 1
                one = [dict(good=[s_["good"][j]], bad=[]) for j in C.FORCED if j < len(s_["good"])]
                res = oracle.variant_read_stats(w["variants"][:1], one, [[1] * len(one)], 20, 11, 0)[0]
                assert res[2] == [1] * len(one) and res[3] == [6 + j % 15 for j in C.FORCED if j < len(s_["good"])]
                n += 1
    assert n >= 8
