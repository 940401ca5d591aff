"""GPU tests of the read-group front ends: plat_bam_route_batch against the rule restated in tests/bam_aux_reference.py (verdicts) and
numpy's stable argsort (the partition), and plat_call_bam_regions_rg / plat_call_bgzf_regions_rg on the fetched fixture's reads as merged
files against plat_call_bam_regions on the pre-split samples of the same reads (the path the existing tests pin to the reference's
lines)."""
import gzip
import json
import os

import numpy as np
import pytest

from platypus_amd import _lib, fastcaller as F, hostapi as H
from platypus_amd.options import default_options
from tests import bam_aux_reference as R
from tests import bgzf_cases as K

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
T = 256                                                      # the partition's tile (ROUTE_TILE of csrc/plat_bamroute.hip)


def _blob(recs, lead=0):
    off = np.cumsum([lead] + [len(r) for r in recs])
    return np.frombuffer(b"\xa5" * lead + b"".join(recs), dtype=np.uint8), off[:-1].astype(np.int64), off[1:].astype(np.int64)


def _check(got, recs, verdicts, stream_begin, n_samples, off, end):
    perm, out_begin, rec_sample, status = R.expected_route(verdicts, stream_begin, n_samples)
    assert got["guard_intact"]
    assert list(got["status"]) == status
    assert np.array_equal(got["out_begin"], out_begin)
    assert np.array_equal(got["rec_sample"], rec_sample)
    assert np.array_equal(got["rec_off"], off[perm]) and np.array_equal(got["rec_limit"], end[perm])
    bad = [v for v, _ in verdicts if v != R.ROUTED]
    assert got["why"] == (bad[0] if bad else 0)


def test_route_gives_the_rule_on_the_hand_made_records():
    eng = H.get_engine()
    cases = R.hand_records()
    recs = [r for _, r in cases]
    table = R.table_of(R.IDS, R.SAMPLES)
    verdicts = [R.verdict(r, table) for r in recs]
    assert {v for v, _ in verdicts} == set(range(8))
    for lead in range(4):
        blob, off, end = _blob(recs, lead)
        got = eng.bam_route(blob, off, end, [0, len(recs)], R.IDS, R.SAMPLES, 3, check=False)
        _check(got, recs, verdicts, [0, len(recs)], 3, off, end)
    # the same records as five streams, two of them empty, and a record capacity above the records in use
    n = len(recs)
    sb = [0, 7, 7, 20, 20, n - 4]
    blob, off, end = _blob(recs, 1)
    got = eng.bam_route(blob, off, end, sb, R.IDS, R.SAMPLES, 3, check=False)
    _check(got, recs[:n - 4], verdicts[:n - 4], sb, 3, off, end)
    # a record whose offsets leave the blob is refused by its fixed part; no table at all: nothing is in it
    got = eng.bam_route(blob, [off[0], -1, off[2], off[3]], [end[0], end[1], len(blob) + 1, off[3] - 1], [0, 4], R.IDS, R.SAMPLES, 3, check=False)
    assert list(got["status"]) == [-9, 1, 1, 3] and got["why"] == R.FIXED_OVERRUN and list(got["rec_sample"]) == [0, -1, -1, -1] and got["guard_intact"]
    got = eng.bam_route(blob, off[:3], end[:3], [0, 3], [], [], 1, check=False)
    assert list(got["status"]) == [-9, 0, 0, 3] and got["why"] == R.NOT_IN_TABLE and got["guard_intact"]


def _ids(n, rng, lo, hi):
    out = set()
    while len(out) < n:
        out.add(bytes(rng.integers(33, 127, size=int(rng.integers(lo, hi + 1)), dtype=np.uint8)))
    return sorted(out)


COUNTS = [0, 1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1]


@pytest.mark.parametrize("n_samples,n_groups,id_len", [(1, 1, (1, 1)), (2, 2, (1, 8)), (3, 300, (1, 40)), (64, 128, (4, 12)), (65, 195, (3, 30)),
                                                        (130, 300, (60, 255))])
def test_route_partitions_streams_stably(n_samples, n_groups, id_len):
    """Streams of 0 .. 2T+1 records, 1 to 130 samples, 1 to 300 groups with one, two and three IDs per sample; the last case's IDs hold
    more bytes than the table keeps in LDS (they are compared in device memory)."""
    eng = H.get_engine()
    rng = np.random.default_rng(n_samples * 1000 + n_groups)
    ids = _ids(n_groups, rng, *id_len)
    assert (sum(len(i) for i in ids) > _lib.ROUTE_LDS_ID_BYTES) == (n_samples == 130)
    samples = [g % n_samples for g in range(n_groups)]
    order = rng.permutation(len(COUNTS))
    sb = np.concatenate([[0], np.cumsum([COUNTS[k] for k in order])])
    n = int(sb[-1])
    groups = rng.integers(0, n_groups, size=n)
    f = R.fixed_part(l_seq=3, n_cig=1, name=b"\0")
    recs = [f + (R.TWELVE[int(g) % 12] if i % 3 == 0 else b"") + R.rg(ids[int(g)]) for i, g in enumerate(groups)]
    table = R.table_of(ids, samples)
    verdicts = [R.verdict(recs[i], table) for i in range(0, n, 97)]
    assert verdicts == [(R.ROUTED, samples[int(groups[i])]) for i in range(0, n, 97)]     # (the restated rule on a sample of them)
    verdicts = [(R.ROUTED, samples[int(g)]) for g in groups]
    blob, off, end = _blob(recs, 2)
    got = eng.bam_route(blob, off, end, sb, ids, samples, n_samples)
    _check(got, recs, verdicts, sb, n_samples, off, end)
    if n_samples == 3:
        # all records in one sample, another with none: every group of the records maps to sample 1
        one = [1 if g in set(groups.tolist()) else 2 for g in range(n_groups)]
        got = eng.bam_route(blob, off, end, sb, ids, one, 3)
        _check(got, recs, [(R.ROUTED, 1)] * n, sb, 3, off, end)
        assert got["out_begin"][1::3].tolist() == sb[:-1].tolist()
        # equal IDs in the table: the lowest index counts
        got = eng.bam_route(blob, off, end, sb, ids + ids, [0] * n_groups + [2] * n_groups, 3)
        _check(got, recs, [(R.ROUTED, 0)] * n, sb, 3, off, end)


def test_route_scans_take_a_second_round():
    """One round of the workgroup scan is 4096 elements: 4100 streams of 0, 1, 2 and T + 1 records (a tile table and, with 3 samples, a
    table of 12 300 stream-sample counts, both longer than one round)."""
    eng = H.get_engine()
    n_streams, n_samples, n_groups = 4100, 3, 6
    rng = np.random.default_rng(n_streams)
    ids = _ids(n_groups, rng, 1, 8)
    samples = [g % n_samples for g in range(n_groups)]
    sb = np.concatenate([[0], np.cumsum([(0, 1, 2, T + 1)[k % 4] for k in range(n_streams)])])
    n = int(sb[-1])
    groups = rng.integers(0, n_groups, size=n)
    f = R.fixed_part(l_seq=3, n_cig=1, name=b"\0")
    by_group = [f + R.rg(i) for i in ids]
    recs = [by_group[int(g)] for g in groups]
    table = R.table_of(ids, samples)
    assert [R.verdict(recs[i], table) for i in range(0, n, 997)] == [(R.ROUTED, samples[int(groups[i])]) for i in range(0, n, 997)]
    blob, off, end = _blob(recs, 2)
    got = eng.bam_route(blob, off, end, sb, ids, samples, n_samples)
    _check(got, recs, [(R.ROUTED, samples[int(g)]) for g in groups], sb, n_samples, off, end)
    assert len(got["out_begin"]) == n_streams * n_samples + 1 and int(got["status"][2]) == n == 1025 * (T + 4)


def test_refusals_name_the_lowest_record_and_route_the_others():
    eng = H.get_engine()
    cases = dict(R.hand_records())
    table = R.table_of(R.IDS, R.SAMPLES)
    bad = {R.NO_RG: "no RG field", R.RG_NOT_STRING: "RG of type i", R.NOT_IN_TABLE: "a prefix of an ID", R.UNKNOWN_TYPE: "unknown B subtype",
           R.NEGATIVE_COUNT: "negative B count", R.AUX_OVERRUN: "RG without NUL", R.FIXED_OVERRUN: "the qualities are cut"}
    good = [R.fixed_part() + R.rg(R.IDS[k % 4]) for k in range(10)]
    for why, name in bad.items():
        assert R.verdict(cases[name], table) == (why, -1)
        for at in (0, 4, 9):
            recs = good[:at] + [cases[name]] + good[at + 1:]
            blob, off, end = _blob(recs, at % 4)
            got = eng.bam_route(blob, off, end, [0, 3, 10], R.IDS, R.SAMPLES, 3, check=False)
            assert list(got["status"]) == [-9, at, 9, 1] and got["why"] == why
            _check(got, recs, [R.verdict(r, table) for r in recs], [0, 3, 10], 3, off, end)
    # several refusals: the lowest is named, all are counted; check=True raises with the rule's name
    recs = good[:2] + [cases["unknown type"]] + good[3:7] + [cases["no aux data"], cases["Z without NUL"]] + good[9:]
    blob, off, end = _blob(recs)
    got = eng.bam_route(blob, off, end, [0, 10], R.IDS, R.SAMPLES, 3, check=False)
    assert list(got["status"]) == [-9, 2, 7, 3] and got["why"] == R.UNKNOWN_TYPE
    with pytest.raises(_lib.PlatypusDeviceError) as e:
        eng.bam_route(blob, off, end, [0, 10], R.IDS, R.SAMPLES, 3)
    assert e.value.code == -9 and "record 2" in str(e.value) and "unknown type" in str(e.value)
    # the limits: one group or one sample more than the kernel takes
    blob, off, end = _blob(good)
    for ids, smp, n_samples in ((_ids(_lib.ROUTE_MAX_GROUPS + 1, np.random.default_rng(1), 3, 3), [0] * (_lib.ROUTE_MAX_GROUPS + 1), 1),
                                (R.IDS, R.SAMPLES, _lib.ROUTE_MAX_SAMPLES + 1)):
        with pytest.raises(_lib.PlatypusDeviceError) as e:
            eng.bam_route(blob, off, end, [0, 10], ids, smp, n_samples)
        assert e.value.code == -6
    # ... and the largest table it takes
    ids = _ids(_lib.ROUTE_MAX_GROUPS, np.random.default_rng(2), 2, 9)
    smp = [g % _lib.ROUTE_MAX_SAMPLES for g in range(len(ids))]
    recs = [R.fixed_part() + R.rg(ids[g]) for g in range(0, len(ids), 7)]
    blob2, off2, end2 = _blob(recs)
    got = eng.bam_route(blob2, off2, end2, [0, len(recs)], ids, smp, _lib.ROUTE_MAX_SAMPLES)
    _check(got, recs, [(R.ROUTED, smp[g]) for g in range(0, len(ids), 7)], [0, len(recs)], _lib.ROUTE_MAX_SAMPLES, off2, end2)
    # arguments the device checks: a sample outside the range, streams that are no partition -- PLAT_ERR_INVALID and nothing written
    for sb, smp in (([0, 10], [0, 1, 3, 1, 2]), ([0, 11], R.SAMPLES), ([1, 10], R.SAMPLES), ([0, 6, 4, 10], R.SAMPLES)):
        got = eng.bam_route(blob, off, end, sb, R.IDS, smp, 3, check=False)
        assert list(got["status"]) == [-1, -1, 0, 0] and got["guard_intact"] and len(got["rec_off"]) == 0
    # the engine is usable afterwards
    got = eng.bam_route(blob, off, end, [0, 10], R.IDS, R.SAMPLES, 3)
    _check(got, good, [R.verdict(r, table) for r in good], [0, 10], 3, off, end)


# ---- the front ends on the goldens ----------------------------------------------------------------------------------------------
def _cases():
    with gzip.open(os.path.join(HERE, "golden", "region_fetched_cases.json.gz"), "rt") as f:
        return json.load(f)


def _rule_end(pos, flag, cigar):
    rec_pos = pos + (cigar[0][1] if cigar and cigar[0][0] == 4 else 0)
    if (flag & 4) or not cigar:
        return rec_pos + 1
    return rec_pos + sum(ln for op, ln in cigar if op in (0, 2, 3, 7, 8))


def _entries(samples, which):
    """The read groups of the samples `which`: two IDs per sample (the first and the second half of its reads, so that the merge keeps the
    sample's own order also among reads of equal position; the broken mates go with the first)."""
    out = []
    for i in which:
        fr, br = samples[i]
        out.append((i, "s%d.a" % i, fr[:len(fr) // 2], br))
        out.append((i, "s%d.b" % i, fr[len(fr) // 2:], []))
    return out


def _groups(n_samples):
    g = [("s%d.%s" % (i, ab), i) for i in range(n_samples) for ab in "ab"]
    return g + [("decoy", n_samples - 1)]                    # (a group no record carries)


def _case_regions(case, ref, ci):
    """The regions of one fixture case for the pre-split call, for both merged-file calls as ONE file, and (2-3 samples) as TWO files."""
    from tests.region_golden import _reads
    fasta = H.FastaFile({"20": case["ref"].encode()})
    nS = len(case["sample_names"])
    bam, one_bam, one_bgz, two_bam, two_bgz = [], [], [], [], []
    kw = dict(level=(1, 6, 9)[ci % 3], block_payload=(0xff00, 4000, 700)[ci % 3], n_chunks=1 + ci % 2)
    for r, rr in zip(case["regions"], ref["regions"]):
        samples = []
        for i, s in enumerate(r["samples"]):
            fr = [K.aligned(x, _rule_end(x["pos"], x["flag"], x["cigar"])) for x in s["fetched"]]
            br = _reads(rr["samples"][i]["brokenMates"]) if rr["loaded"] else []
            for b in br:
                b.end = _rule_end(b.pos, b.bitFlag, b.cigarOps)
            samples.append((fr, br))
        at = (r["chrom"], r["start"], r["end"], fasta)
        bam.append(F.BamRegion.from_reads(*at, samples))
        merged = [_entries(samples, range(nS))]
        one_bam.append(F.BamFileRegion.from_reads(*at, merged))
        one_bgz.append(F.BgzfFileRegion.from_reads(*at, merged, **kw))
        if nS > 1:
            halves = [_entries(samples, range(0, nS, 2)), _entries(samples, range(1, nS, 2))]
            two_bam.append(F.BamFileRegion.from_reads(*at, halves))
            two_bgz.append(F.BgzfFileRegion.from_reads(*at, halves, **kw))
    return bam, one_bam, one_bgz, two_bam, two_bgz


def _same_as_pre_split(nc, case, options, regions, ci):
    """Both new calls on every variant against plat_call_bam_regions on the pre-split samples; returns (text, loaded, variants run)."""
    bam, one_bam, one_bgz, two_bam, two_bgz = regions
    nS = len(case["sample_names"])
    o1 = default_options(**options)
    want = nc.call_bam_regions(bam, case["sample_names"], o1)
    want_loaded, want_counts, want_lens = list(nc.loaded), nc.read_counts.copy(), nc.region_text_lengths(len(bam)).copy()
    n = 0
    for regs, call in ((one_bam, nc.call_bam_regions_rg), (one_bgz, nc.call_bgzf_regions_rg), (two_bam, nc.call_bam_regions_rg),
                       (two_bgz, nc.call_bgzf_regions_rg)):
        if not regs:
            continue
        o2 = default_options(**options)
        got = call(regs, _groups(nS), case["sample_names"], o2)
        assert got == want, ci
        assert o2.rlen == o1.rlen, ci
        assert nc.loaded == want_loaded, ci
        assert np.array_equal(nc.read_counts, want_counts), ci
        assert np.array_equal(nc.region_text_lengths(len(regs)), want_lens), ci
        n += 1
    return want, want_loaded, n


def _golden():
    cases = _cases()
    with gzip.open(os.path.join(HERE, "golden", "region_cases.json.gz"), "rt") as f:
        after = json.load(f)
    return cases, after


def test_merged_files_equal_the_pre_split_call_on_all_cases():
    """All 41 cases of the fetched fixture as ONE merged file per region, two read-group IDs per sample and a decoy group, through both new
    calls: text, rlen, loaded, per-sample counts and region text lengths are those of plat_call_bam_regions on the pre-split samples.  The
    twelve cases with 2-3 samples (10 480 fetched reads) go through them again as TWO files, the samples dealt out between them."""
    cases, after = _golden()
    assert len(cases) == 41
    multi = [c for c in cases if len(c["sample_names"]) > 1]
    assert len(multi) == 12 and {len(c["sample_names"]) for c in multi} == {2, 3}
    assert sum(len(s["fetched"]) for c in multi for r in c["regions"] for s in r["samples"]) == 10480
    nc = F.NativeCaller(0, 2, 2)
    n_lines = n_two = 0
    try:
        for ci, (case, ref) in enumerate(zip(cases, after)):
            want, loaded, n = _same_as_pre_split(nc, case, case["options"], _case_regions(case, ref, ci), ci)
            assert loaded == [int(r["loaded"]) for r in case["regions"]], ci
            n_lines += want.count("\n")
            n_two += n == 4
    finally:
        nc.close()
    assert n_lines > 200 and n_two == 12


def test_max_reads_drops_a_region_next_to_a_loaded_one():
    """Two two-sample cases' regions in one call (656 and 473 fetched reads), maxReads = 656: the first region is dropped, the second loads
    -- the BGZF call's second find and second route run over the loaded region alone."""
    cases, after = _golden()
    pair = (1, 15)
    assert [sum(len(s["fetched"]) for s in cases[ci]["regions"][0]["samples"]) for ci in pair] == [656, 473]
    assert all(len(cases[ci]["sample_names"]) == 2 and len(cases[ci]["regions"]) == 1 and not cases[ci]["options"] for ci in pair)
    parts = [_case_regions(cases[ci], after[ci], ci) for ci in pair]
    regions = tuple(parts[0][k] + parts[1][k] for k in range(5))
    nc = F.NativeCaller(0, 2, 2)
    try:
        want, loaded, n = _same_as_pre_split(nc, cases[1], dict(maxReads=656), regions, pair)
    finally:
        nc.close()
    assert n == 4 and loaded == [0, 1] and want.count("\n") > 0


def test_refused_records_and_unsorted_streams_surface_through_the_front_ends():
    ref = b"ACGTTGCA" * 100
    fasta = H.FastaFile({"20": ref})
    rd = lambda p: H.AlignedRead(ref[p:p + 60], bytes([30] * 60), p, bitFlag=3)
    groups = {"lane1": 0, "lane2": 1}
    names = ["S1", "S2"]
    a, b = [rd(p) for p in (100, 140, 180, 220)], [rd(p) for p in (120, 160, 200)]
    entries = [(0, "lane1", a, []), (1, "lane2", b, [])]
    at = ("20", 100, 500, fasta)
    nc = F.NativeCaller(0, 1, 2)
    try:
        want = nc.call_bam_regions([F.BamRegion.from_reads(*at, [(a, []), (b, [])])], names, default_options())
        for cls, call, unit in ((F.BamFileRegion, nc.call_bam_regions_rg, 1), (F.BgzfFileRegion, nc.call_bgzf_regions_rg, 1)):
            good = cls.from_reads(*at, [entries])
            assert call([good], groups, names, default_options()) == want
            # an ID the table does not hold: record 3 of the merged file (100 120 140 160 ...) is lane2's second
            stranger = cls.from_reads(*at, [[(0, "lane1", a, []), (1, "lane9", b[1:2], []), (1, "lane2", b[:1] + b[2:], [])]])
            with pytest.raises(_lib.PlatypusDeviceError) as e:
                call([good, stranger], groups, names, default_options())
            msg = str(e.value)
            assert e.value.code == -9 and "region 1" in msg and "file 0" in msg and "fetched record 3 " in msg and "not in the table" in msg
            assert call([good], groups, names, default_options()) == want
            # a sample split over two files so that its stream is not sorted: file 0 holds its later reads
            halves = cls.from_reads(*at, [[(0, "lane1", a[2:], []), (1, "lane2", b, [])], [(0, "lane1", a[:2], [])]])
            with pytest.raises(_lib.PlatypusDeviceError) as e:
                call([halves], groups, names, default_options())
            assert e.value.code == -9 and "not sorted by position" in str(e.value) and "sample 0" in str(e.value)
            # ... and in file order it is the pre-split call
            halves = cls.from_reads(*at, [[(0, "lane1", a[:2], []), (1, "lane2", b, [])], [(0, "lane1", a[2:], [])]])
            assert call([halves], groups, names, default_options()) == want
        # a record without an RG field (the raw-record call: its aux bytes are the caller's): record 2 of file 0 loses its field, and its
        # rec_len says so
        good = F.BamFileRegion.from_reads(*at, [entries])
        (data, off, ln), broken = good.files[0]
        cut = len(b"RGZlane1\0")
        keep = np.ones(len(data), dtype=bool)
        keep[off[2] + ln[2] - cut:off[2] + ln[2]] = False
        ln2, off2 = ln.copy(), off.copy()
        ln2[2] -= cut
        off2[3:] -= cut
        bare = F.BamFileRegion("20", 100, 500, ref, [((data[keep], off2, ln2), broken)])
        with pytest.raises(_lib.PlatypusDeviceError) as e:
            nc.call_bam_regions_rg([good, good, bare], groups, names, default_options())
        msg = str(e.value)
        assert e.value.code == -9 and "region 2" in msg and "file 0" in msg and "fetched record 2 " in msg and "no RG field" in msg
        # the table's own checks
        for bad, what in (([("lane1", 0), ("lane1", 1), ("lane2", 1)], "twice"), ([("lane1", 0), ("lane2", 2)], "sample 2"), ([("", 0)], "empty")):
            with pytest.raises(_lib.PlatypusDeviceError) as e:
                nc.call_bam_regions_rg([good], bad, names, default_options())
            assert e.value.code == -1 and what in str(e.value)
        short = F.BamFileRegion("20", 100, 500, ref, [((data, off, np.minimum(ln, 31)), broken)])
        with pytest.raises(_lib.PlatypusDeviceError) as e:
            nc.call_bam_regions_rg([short], groups, names, default_options())
        assert e.value.code == -1 and "rec_len" in str(e.value)
        assert nc.call_bam_regions_rg([good], groups, names, default_options()) == want
    finally:
        nc.close()
