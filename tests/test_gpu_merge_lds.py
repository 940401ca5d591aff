"""plat_candidates_merge_batch as one kernel per chunk (one workgroup per scan, the hash table in LDS, the filter fused): the shapes at
which that structure can go wrong.  Expectations are the reference's dictionary step and support filter as _merge_expected of
test_gpu_stage_b_kernels.py computes them (variant.pyx:499-527, variantcaller.pyx:456-467, hostapi.ReadArray.countReadsCoveringRegion)
from the scan's records -- never another device path.  Rows are compared as sets; out_n, the rep ids and the sentinel behind the count
exactly.  Each test is a few launches."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stage_b_reference as R  # noqa: E402
from test_gpu_stage_b_kernels import _StopOnDeviceError, _flip, _merge_expected  # noqa: E402
from platypus_amd import hostapi as H  # noqa: E402
from platypus_amd.engine import Engine  # noqa: E402

pytestmark = pytest.mark.gpu

# what the kernel is built around (csrc/plat_candidates.hip), restated: a change there has to revisit the shapes below
MERGE_SLOTS, MERGE_LIMIT = 8192, 6144
MERGE_QUEUE = 8192                                                               # records per round of collect + insert
MERGE_STRIDE = 1024 * 4                                                          # reads per trip of the workgroup's collect phase
SENT = Engine.sentinel_of("i4")


@pytest.fixture(scope="module")
def eng():
    return _StopOnDeviceError(H.get_engine())


def _read(seq, pos, cigar=None, end=None):
    seq = bytes(seq)
    return dict(seq=seq, qual=b"\x28" * len(seq), pos=pos, flag=3, cigar=cigar or [(0, len(seq))], end=pos + len(seq) if end is None else end)


def _snp_read(ref, pos, length, sites, alt=_flip):
    """A read of ref[pos:pos + length] with the bases at the absolute positions `sites` exchanged."""
    seq = bytearray(ref[pos:pos + length])
    for p in sites:
        seq[p - pos] = alt(seq[p - pos])
    return _read(seq, pos)


def _merge(eng, regs, begin, max_per_read, thr, cap, ends=None):
    """Scan `regs`, merge the scans `begin` cuts its reads into, compare everything with the reference's dictionary step.
    -> (cand, n, want, last_candidates)"""
    eng.candidates(regs, max_per_read=max_per_read, retry=False, keep_device=True)
    lc = eng.last_candidates
    reads = [r for g in regs for r in g["reads"]]
    longest = [max([r["end"] - r["pos"] for r in reads[begin[g]:begin[g + 1]]], default=0) for g in range(len(begin) - 1)]
    cand, n = eng.candidates_merge(begin, [r["end"] for r in reads] if ends is None else ends, longest, thr, cap)
    blob = lc["read_seq"].tobytes()
    want = _merge_expected(regs, begin, lc["rec"], lc["count"], max_per_read, lambda ao, k: blob[ao:ao + k], thr)
    return cand, n, want, lc


def _check(cand, n, want, lc, max_per_read, refused=()):
    for g in range(len(want)):
        if g in refused:
            continue
        assert n[g].tolist() == [len(want[g]), 0], (g, n[g].tolist(), len(want[g]))
        rows = cand[g, :n[g, 0]]
        assert {tuple(r[:6].tolist()) for r in rows} == want[g], g
        assert len({int(r[0]) for r in rows}) == len(rows), (g, "a content twice")
        for r in rows:                                                           # the rep's own record
            assert r[3:8].tolist() == lc["rec"][r[0] // max_per_read, r[0] % max_per_read].tolist()
        assert (cand[g, n[g, 0]:] == SENT).all(), (g, "rows behind out_n keep the sentinel")


def _begin(regs):
    return np.concatenate([[0], np.cumsum([len(g["reads"]) for g in regs])]).tolist()


def _region(ref, reads):
    return dict(ref=ref, ref_seq_start=0, contig_len=len(ref), reads=reads)


def test_a_scan_of_three_queue_rounds_keeps_the_first_record_as_rep(eng):
    """640 reads at one position, 40 sites each 12 apart, read i shows site s unless (i + s) % 3 == 0: 17 066 records, three rounds of
    the queue; each of the 40 contents occurs in every round, its rep is the record of read 0 or 1."""
    ref = R.synth_ref(1200, 31)
    L = 30 + 12 * 40
    sites = [115 + 12 * s for s in range(40)]
    reads = [_snp_read(ref, 100, L, [p for s, p in enumerate(sites) if (i + s) % 3]) for i in range(640)]
    regs = [_region(ref, reads), _region(ref, [_snp_read(ref, 100, L, sites[:3])])]
    cand, n, want, lc = _merge(eng, regs, _begin(regs), 64, 0.05, 48)
    assert int(lc["count"][:640].sum()) == sum(1 for i in range(640) for s in range(40) if (i + s) % 3) > 2 * MERGE_QUEUE
    _check(cand, n, want, lc, 64)
    assert n[0].tolist() == [40, 0] and n[1].tolist() == [3, 0]
    rows = sorted(cand[0, :40].tolist())
    assert [r[0] // 64 for r in rows] == [0] * 26 + [1] * 14                     # read 0 lacks the 14 sites s % 3 == 0: read 1 shows those first
    assert sorted(r[1] for r in rows) == sorted(sum(1 for i in range(640) if (i + s) % 3) for s in range(40))
    assert all(r[2] == 640 for r in rows)


def test_scans_longer_than_a_stride_and_shorter_than_a_wave_beside_empty_ones(eng):
    """One call: 5 000 reads (more than one trip of the workgroup over its reads) | no read | one read | 40 reads | no read | one read."""
    ref = R.synth_ref(3200, 43)
    big = []
    for i in range(5000):
        pos = 100 + (i * 2800) // 5000
        sites = [p for p in range(pos + 12, pos + 88) if p % 50 == 0 and (i % 7 == 0 or p % 250 == 0)]   # shared sites, some shown by few reads
        if i % 5 == 0:
            sites.append(pos + 20 + (i // 5) % 60)                               # ... and errors of single reads
        big.append(_snp_read(ref, pos, 100, sorted(set(sites))))
    assert len(big) > MERGE_STRIDE
    small = [_snp_read(ref, 400 + 2 * i, 120, [470, 482] if i % 2 else [470]) for i in range(40)]
    one = [_snp_read(ref, 900, 100, [950])]
    regs = [_region(ref, big), _region(ref, []), _region(ref, one), _region(ref, small), _region(ref, []), _region(ref, one)]
    for thr in (0.05, 0.5):
        cand, n, want, lc = _merge(eng, regs, _begin(regs), 16, thr, 1024)
        _check(cand, n, want, lc, 16)
        assert n[1].tolist() == [0, 0] and n[4].tolist() == [0, 0] and n[2].tolist() == [1, 0] and n[5].tolist() == [1, 0]
        assert cand[5, 0, :3].tolist() == [16 * 5041, 1, 1]
    assert len(want[0]) < int(lc["count"][:5000].sum())                          # (the threshold of 0.5 removes some)


def _slot(pos, rem, add):
    """The kernel's hash of a record's content and the slot its probe starts at."""
    m = 0xFFFFFFFF
    h = (pos * 2654435761 + len(rem) * 40503 + len(add) * 97) & m
    for b in rem:
        h = (h * 31 + b) & m
    for b in add:
        h = (h * 37 + b) & m
    return (h ^ (h >> 15)) & (MERGE_SLOTS - 1)


def test_contents_that_differ_in_one_byte_or_one_length_and_a_probe_run_of_one_slot(eng):
    ref = R.synth_ref(1200, 47)
    at = 300                                                                     # 8 inserted bases behind ref[at + 59]: the records' position is at + 59
    by_slot = {}
    for v in range(4 ** 8):
        ins = bytes(b"ACGT"[(v >> (2 * k)) & 3] for k in range(8))
        by_slot.setdefault(_slot(at + 59, b"", ins), []).append(ins)
    run = max(by_slot.values(), key=len)
    assert len(run) >= 8 and len({_slot(at + 59, b"", x) for x in run}) == 1    # 65 536 contents over 8 192 slots
    run = run[:8]
    last = run[0][:7] + bytes([_flip(run[0][7])])                                # the first of them with another last byte
    ins_read = lambda ins: _read(ref[at:at + 60] + ins + ref[at + 60:at + 120], at, [(0, 60), (1, 8), (0, 60)], at + 120)
    del_read = lambda k: _read(ref[at:at + 60] + ref[at + 60 + k:at + 120 + k], at, [(0, 60), (2, k), (0, 60)], at + 120 + k)
    mnp = lambda a, b, c: _snp_read(ref, at, 120, [at + 30, at + 31, at + 32], alt=lambda x, it=iter((a, b, c)): [y for y in b"ACGT" if y != x][next(it)])
    reads = []
    for rep in range(3):                                                         # every content three times, the order turned round in between
        order = run + [last]
        for ins in (order if rep != 1 else order[::-1]):
            reads.append(ins_read(ins))
    reads += [del_read(2), del_read(3), del_read(2), del_read(4)]                # equal position, nothing added: the removed length alone tells them apart
    reads += [mnp(0, 1, 0), mnp(0, 1, 1), mnp(0, 1, 0), mnp(0, 1, 2)]            # three bases exchanged, the last one three ways
    regs = [_region(ref, reads), _region(ref, reads[:9])]
    cand, n, want, lc = _merge(eng, regs, _begin(regs), 8, 0.0, 64)
    _check(cand, n, want, lc, 8)
    rows = cand[0, :n[0, 0]].tolist()
    blob = lc["read_seq"].tobytes()
    ins_rows = {blob[r[7]:r[7] + 8]: r for r in rows if (r[4], r[5]) == (0, 8)}
    assert set(ins_rows) == set(run + [last]) and all(r[1] == 3 and r[3] == at + 59 for r in ins_rows.values())
    assert [ins_rows[x][0] for x in run + [last]] == [8 * k for k in range(9)]   # rep = the first read that shows it
    assert sorted((r[4], r[1]) for r in rows if r[5] == 0) == [(2, 2), (3, 1), (4, 1)]
    assert sorted(r[1] for r in rows if (r[4], r[5]) == (3, 3)) == [1, 1, 2]
    assert n[1].tolist() == [9, 0]


def test_exactly_merge_limit_distinct_records_are_taken_and_one_more_is_refused(eng):
    """Groups of 12 reads, one base apart, 40 sites each 12 apart: 480 distinct positions per group, groups 520 apart.  6 144 distinct
    records = 153 reads of 40 sites and one of 24; the scan beside it has one site more."""
    ref = R.synth_ref(8200, 53)
    L = 30 + 12 * 40

    def scan(n_distinct):
        reads, keys = [], set()
        i = 0
        while len(keys) < n_distinct:
            pos = 100 + 520 * (i // 12) + i % 12
            sites = [pos + 15 + 12 * s for s in range(min(40, n_distinct - len(keys)))]
            keys |= set(sites)
            reads.append(_snp_read(ref, pos, L, sites))
            i += 1
        assert len(keys) == n_distinct and sum(len(r["seq"]) == L for r in reads) == len(reads) <= 200
        return reads
    regs = [_region(ref, scan(MERGE_LIMIT)), _region(ref, scan(40)), _region(ref, scan(MERGE_LIMIT + 1)), _region(ref, scan(41))]
    begin = _begin(regs)
    eng.candidates(regs, max_per_read=64, retry=False, keep_device=True)
    lc = eng.last_candidates
    blob = lc["read_seq"].tobytes()
    distinct = []
    for g in range(4):                                                           # the construction, counted on the host before the merge sees it
        keys = set()
        for r in range(begin[g], begin[g + 1]):
            assert lc["status"][r] == 0 and lc["count"][r] <= 40
            keys |= {(int(p), int(a), int(b), blob[ao:ao + b]) for p, a, b, _, ao in lc["rec"][r, :lc["count"][r]]}
        distinct.append(len(keys))
    assert distinct == [MERGE_LIMIT, 40, MERGE_LIMIT + 1, 41]
    cap = MERGE_LIMIT + 8
    cand, n, want, lc = _merge(eng, regs, begin, 64, 0.0, cap)
    _check(cand, n, want, lc, 64, refused=(2,))
    assert n[:, 0].tolist() == [MERGE_LIMIT, 40, 0, 41]
    assert n[2].tolist() == [0, R.ERR_OVERFLOW] and (cand[2] == SENT).all()      # a refused scan writes no row


def _replay_case(eng, first):
    """The region of test_two_alleles_of_equal_support_are_ordered_by_the_replayed_dictionaries, merged and taken through stage B with the
    scan's records; `first`: a call made on the same context just before."""
    from platypus_amd.vcfrecords import _py2_string_hash
    ref = R.synth_ref(1500, 41)
    sites = [500, 620, 700, 810]
    reads = []
    for k in range(24):
        pos = 380 + 20 * k
        seq = bytearray(ref[pos:pos + 150])
        for j, p in enumerate(sites):
            if pos + 12 <= p < pos + 138:
                alts = [b for b in b"ACGT" if b != ref[p]]
                seq[p - pos] = alts[(k + j) % 2] if j < 3 else alts[0]
        reads.append(_read(seq, pos))
    regs = [_region(ref, reads)]
    first()
    cand, n, want, lc = _merge(eng, regs, [0, len(reads)], 16, 0.05, 32)
    _check(cand, n, want, lc, 16)
    assert n[0].tolist() == [7, 0]
    blob = lc["read_seq"].tobytes()
    rows = sorted(cand[0, :7].tolist())
    cands = [(r[3], r[4], blob[r[7]:r[7] + r[5]], r[1], r[0]) for r in rows]
    distinct, seen = [], {}
    for r in range(len(reads)):
        for k in range(lc["count"][r]):
            pos, nrem, nadd, ro, ao = lc["rec"][r, k].tolist()
            key = (pos, ref[ro:ro + nrem], blob[ao:ao + nadd])
            if key not in seen:
                seen[key] = len(distinct)
                rid = r * 16 + k
                distinct.append(key + (next((i for i, c in enumerate(cands) if c[4] == rid), None),))
    reg = R.region(ref, cands, rlen=150, start=400, end=1000, reads=[(r["pos"], r["end"], len(r["seq"])) for r in reads])
    a = R.pack([reg])
    h = _py2_string_hash("20")
    gd = [dict(start=400, end=1000, rlen=150, name_hash=h - (1 << 64) if h >= 1 << 63 else h)]
    o, cp = R.options(), R.caps()
    out = eng.stage_b(gd, a["tables"], o, with_records=True, **cp)
    exp = R.expected([reg], o, cp, 32, exact_records=[distinct])
    assert exp["regions"][0]["replay"] == 1 and exp["regions"][0]["status"] == 0
    R.compare(out, exp, [reg], cp, Engine.sentinel_of)
    assert out["hdr"][0, 6] == 1 and out["hdr"][0, 1] == 7


def test_a_second_call_with_fewer_and_smaller_scans_shows_nothing_of_the_first(eng):
    """The table the replay reads is written in full by every call: the first call leaves 2 000 distinct records in scan 0's table (and
    more scans behind it), the second has one scan of 24 reads whose region needs the replay."""
    ref = R.synth_ref(3000, 59)

    def first():
        regs = []
        for g in range(3):
            reads = [_snp_read(ref, 100 + 520 * (i // 12) + i % 12, 510, [100 + 520 * (i // 12) + i % 12 + 15 + 12 * s for s in range(40)]) for i in range(50)]
            regs.append(_region(ref, reads))
        cand, n, want, lc = _merge(eng, regs, _begin(regs), 64, 0.0, 2048)
        _check(cand, n, want, lc, 64)
        assert n[:, 0].tolist() == [2000] * 3
    _replay_case(eng, first)
    _replay_case(eng, lambda: None)                                              # ... and the same case again behind itself


def test_coverage_where_reads_end_at_the_site_and_where_the_key_clamps_to_one(eng):
    """A site at 12 under reads of up to 100 bases: start - longest <= 1, the lower bound is taken for 1 (reads at position 0 lie in front
    of it).  Reads that end exactly at the site: in front of every covering read they are walked over, behind one they count."""
    ref = R.synth_ref(600, 61)
    reads = [_snp_read(ref, 0, 100, [12]), _snp_read(ref, 0, 100, []),
             _read(ref[1:12], 1),                                                # ends at 12, first behind the bound: walked over
             _read(ref[1:12], 1),
             _snp_read(ref, 1, 100, [12]),                                       # shows the site at its index 11
             _read(ref[2:12], 2),                                                # ends at 12 behind a covering read: the reference's loop counts it
             _snp_read(ref, 2, 100, [12]), _snp_read(ref, 2, 60, []),
             _snp_read(ref, 12, 100, [30]),                                      # starts at the site: covers it
             _snp_read(ref, 13, 100, [30])]                                      # starts behind it
    regs = [_region(ref, reads)]
    ra = H.ReadArray([H.AlignedRead(r["seq"], r["qual"], r["pos"], end=r["end"]) for r in reads])
    assert ra.getLengthOfLongestRead() == 100 and (ra.countReadsCoveringRegion(12, 13), ra.countReadsCoveringRegion(30, 31)) == (5, 6)
    for thr in (0.05, 0.5, 0.7):
        cand, n, want, lc = _merge(eng, regs, [0, len(reads)], 8, thr, 8)
        _check(cand, n, want, lc, 8)
        got = {(r[3], r[1], r[2]) for r in cand[0, :n[0, 0]].tolist()}
        assert got == {k for k in ((12, 3, 5), (30, 2, 6)) if float(k[1]) / k[2] >= thr}
    # reads of 40 bases, sites at 41 and 42: start - longest = 1, the bound itself, and 2, the first key that is not clamped
    reads = [_snp_read(ref, 0, 40, []), _snp_read(ref, 1, 40, []),               # the second ends at 41
             _snp_read(ref, 2, 40, []),                                          # ends at 42, covers 41
             _snp_read(ref, 20, 40, [41]), _snp_read(ref, 21, 40, [42]), _snp_read(ref, 25, 40, [41]), _snp_read(ref, 26, 40, [42]),
             _snp_read(ref, 41, 40, []), _snp_read(ref, 42, 40, []), _snp_read(ref, 43, 40, [])]
    ra = H.ReadArray([H.AlignedRead(r["seq"], r["qual"], r["pos"], end=r["end"]) for r in reads])
    assert ra.getLengthOfLongestRead() == 40 and (ra.countReadsCoveringRegion(41, 42), ra.countReadsCoveringRegion(42, 43)) == (6, 6)
    cand, n, want, lc = _merge(eng, [_region(ref, reads)], [0, len(reads)], 8, 0.05, 8)
    _check(cand, n, want, lc, 8)
    assert {(r[3], r[1], r[2]) for r in cand[0, :n[0, 0]].tolist()} == {(41, 2, 6), (42, 2, 6)}
