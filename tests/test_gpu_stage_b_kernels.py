"""plat_candidates_merge_batch and plat_stage_b_batch called directly (Engine.candidates_merge / Engine.stage_b), array by array, against
the committed goldens and tests/stage_b_reference.py (the mirror chain, proven against the same goldens without a GPU by
tests/test_stage_b_reference_cpu.py) -- never against PLAT_CALLER_HOST_B or another device path.  All integers and bytes: every
comparison is exact.  Each test is one or a few launches on small inputs.

R.compare() is run on EVERY call of this file: hdr (status AND reason code as predicted from the inputs), every variant / window /
batch array by content, and the sentinel in every element behind what the counts say was written."""
import gzip
import json
import os
import sys
from itertools import combinations

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stage_b_reference as R  # noqa: E402
from platypus_amd import _lib, hostapi as H  # noqa: E402
from platypus_amd.engine import Engine  # noqa: E402

pytestmark = pytest.mark.gpu

PLAT_ERR_HIP = -2
TALLY = {}                                                                       # what each test compared (printed: profiles/r08_stage_b_kernels.md)


class _StopOnDeviceError:
    """The engine, with one rule added: a HIP error (PLAT_ERR_HIP from the library, or a RuntimeError of torch's whose text names a HIP
    error -- a fault included) ends the session: nothing more is started on that device.  Every other exception is the test's own."""

    def __init__(self, engine):
        self._engine = engine

    def __getattr__(self, name):
        attr = getattr(self._engine, name)
        if not callable(attr):
            return attr

        def call(*args, **kw):
            try:
                return attr(*args, **kw)
            except _lib.PlatypusDeviceError as exc:
                if exc.code == PLAT_ERR_HIP:
                    pytest.exit("device error in Engine.%s: %s" % (name, exc), returncode=3)
                raise
            except RuntimeError as exc:
                if "HIP error" in str(exc) or "hipError" in str(exc):
                    pytest.exit("device error in Engine.%s: %s" % (name, exc), returncode=3)
                raise
        return call


@pytest.fixture(scope="module")
def eng():
    return _StopOnDeviceError(H.get_engine())


@pytest.fixture(scope="module")
def regionprep(golden_dir):
    return json.load(gzip.open(os.path.join(golden_dir, "regionprep_cases.json.gz"), "rt"))


def run(eng, regions, o, cp, cap_per_scan=None, name=None):
    """One plat_stage_b_batch call on hand-made candidates, compared with the expectation in full.  -> (arrays, expectation)"""
    a = R.pack(regions, cap_per_scan)
    out = eng.stage_b(a["regions"], a["tables"], o, cand=a["cand"], cand_n=a["cand_n"], read_seq=a["read_seq"], cap_per_scan=a["cap_per_scan"], **cp)
    exp = R.expected(regions, o, cp, a["cap_per_scan"])
    R.compare(out, exp, regions, cp, Engine.sentinel_of)
    if name:
        t = TALLY.setdefault(name, dict(calls=0, regions=0, flagged=0, variants=0, windows=0, batch_windows=0, haplotypes=0))
        t["calls"] += 1
        for k, v in R.counts(exp).items():
            t[k] += v
        print("[stage-b kernels] %s: %s" % (name, json.dumps(t)))
    return out, exp


# ---- b. normalisation ------------------------------------------------------------------------------------------------------------------------

def test_normalisation_of_the_golden_variants(eng, regionprep):
    """left_normalise: 1 000 regions of one candidate each in one call; var_pos, removed and added bytes, bamMinPos / bamMaxPos and the
    support must be the golden `out`; the regions flagged are exactly the three contig-end indels the documented rule predicts."""
    cases = R.normalise_cases(regionprep)
    regions = [reg for reg, _ in cases]
    o, cp = R.options(**R.NORMALISE_OPTIONS), R.caps(**R.NORMALISE_CAPS)
    out, exp = run(eng, regions, o, cp, name="normalisation, golden")
    eligible = [c[0][1] != len(c[0][2]) and not (c[0][1] and c[0][2]) and c[0][0] >= 100 for c in (reg["cands"] for reg in regions)]
    flagged = [g for g in range(len(regions)) if out["hdr"][g, 0] != 0]
    assert flagged == [g for g, e in enumerate(exp["regions"]) if e["status"]] and all(out["hdr"][g, 5] == 1 and eligible[g] for g in flagged)
    assert (len(cases), sum(eligible), len(flagged)) == (R.N_NORMALISE, R.N_NORMALISE_ELIGIBLE, R.N_NORMALISE_FLAGGED)
    assert len(flagged) <= 0.01 * sum(eligible)
    moved = 0
    for g, (reg, v) in enumerate(cases):
        if g in flagged:
            continue
        assert out["hdr"][g].tolist()[:3] == [0, 1, 1]
        pos, nrem, nadd = int(out["var_pos"][g, 0]), int(out["var_nrem"][g, 0]), int(out["var_nadd"][g, 0])
        rp, ao = int(out["var_rem_pos"][g, 0]), int(out["var_add_off"][g, 0])
        got = [pos, reg["ref"][rp:rp + nrem].decode() if nrem else "", out["added"][g, ao:ao + nadd].tobytes().decode(), int(out["var_bam_min"][g, 0]),
               int(out["var_bam_max"][g, 0]), int(out["var_support"][g, 0])]
        assert got == v["out"][:6], (g, v, got)
        moved += pos != v["pos"]
    assert moved == R.N_NORMALISE_MOVED - R.N_NORMALISE_FLAGGED                 # (each of the three flagged ones is one the reference moves)


def _run_of(unit, n_units, at=600, total=1500, seed=1):
    """A reference with `unit` repeated n_units times from `at`, flanked by bases that end the repeat."""
    ref = bytearray(R.synth_ref(total, seed))
    ref[at:at + len(unit) * n_units] = unit * n_units
    for p in (at - 1, at + len(unit) * n_units):
        ref[p] = next(c for c in b"ACGT" if c not in unit and c != ref[p - 1])
    return bytes(ref)


def test_normalisation_walks_longer_than_one_ballot_step(eng):
    """A deletion and an insertion of one repeat unit reported at the RIGHT end of a homopolymer / dinucleotide run of 63, 64, 65 and 130
    bases: the walk to the left end takes one, two and three 64-lane steps."""
    regions, want = [], []
    for unit in (b"A", b"CT"):
        for n in (63, 64, 65, 130):
            units = n // len(unit)
            ref = _run_of(unit, units)
            end = 600 + len(unit) * units
            regions.append(R.region(ref, [(end - len(unit) - 1, len(unit), b"", 3)], rlen=150))      # the last unit deleted
            regions.append(R.region(ref, [(end - 1, 0, unit, 3)], rlen=150))                          # one more unit behind the last
            want += [599, 599]
    out, exp = run(eng, regions, R.options(), R.caps(cap_vars=4, cap_windows=4, cap_added=8), name="normalisation, long walks")
    assert [int(out["var_pos"][g, 0]) for g in range(len(regions))] == want
    assert all(out["var_bam_max"][g, 0] > out["var_bam_min"][g, 0] + 60 for g in range(len(regions)))


def test_normalisation_edges(eng):
    """refPos 99 / 100; a window cut at wmin = 1; a reference window that starts behind wmin (flagged) or exactly at it; one that ends
    exactly at wmax, and one byte earlier (flagged); the contig's end."""
    ref = _run_of(b"A", 30, at=85, total=900)
    regions = [R.region(ref, [(99, 1, b"", 2)], rlen=100),                       # 0: refPos 99: returned as it is
               R.region(ref, [(100, 1, b"", 2)], rlen=100),                      # 1: refPos 100: moved to the run's left end
               R.region(_run_of(b"A", 110, at=5, total=900), [(113, 1, b"", 2)], rlen=150)]       # 2: wmin = 1 cuts the window inside the run
    contig = _run_of(b"G", 12, at=700, total=3000, seed=4)
    w = 1 + 150                                                                   # max(nAdded, nRemoved) + rlen
    for rss in (710 - w, 710 - w + 1):                                           # 3: the window starts at wmin; 4: one base behind it (flagged)
        regions.append(R.region(contig[rss:1400], [(710, 1, b"", 2)], rlen=150, ref_seq_start=rss, contig_len=3000, start=rss, end=1400))
    for stop in (710 + w, 710 + w - 1):                                          # 5: the window ends at wmax; 6: one base earlier (flagged)
        regions.append(R.region(contig[300:stop], [(710, 1, b"", 2)], rlen=150, ref_seq_start=300, contig_len=3000, start=300, end=stop))
    regions.append(R.region(contig[:800], [(796, 2, b"", 2)], rlen=150))         # 7: the deletion's tail is empty at the contig's end (flagged)
    regions.append(R.region(contig[:800], [(795, 2, b"", 2)], rlen=150))         # 8: one base of tail
    out, exp = run(eng, regions, R.options(), R.caps(cap_vars=4, cap_windows=4, cap_added=8), name="normalisation, edges")
    assert out["hdr"][:, 0].tolist() == [0, 0, 0, 0, 1, 0, 1, 1, 0] and out["hdr"][[4, 6, 7], 5].tolist() == [1, 1, 1]
    assert [int(out["var_pos"][g, 0]) for g in (0, 1, 2, 3, 5)] == [99, 84, 4, 699, 699]


def test_added_bases_fill_cap_added_exactly_and_one_byte_more_is_refused(eng):
    ref = bytearray(_run_of(b"T", 20, at=300, total=900))
    ref[500:512] = b"ACGACGACGACG"
    ref[499:500], ref[512:513] = b"T", b"T"
    cands = [(319, 0, b"TTTTT", 3), (511, 0, b"ACGACGA"[:6], 3), (40, 0, b"GGCA", 3), (60, 1, b"C" if ref[60:61] != b"C" else b"G", 3)]
    need = 5 + 6 + 4 + 1
    for cap, status in ((need, 0), (need - 1, 1)):
        out, exp = run(eng, [R.region(bytes(ref), cands, rlen=100)], R.options(), R.caps(cap_added=cap), name="normalisation, cap_added")
        assert out["hdr"][0, 0] == status and out["hdr"][0, 5] == (6 if status else 0)
        if not status:
            assert out["hdr"][0, 4] == need and sorted(out["var_pos"][0, :4].tolist()) == [40, 60, 299, 499]
    # the moved insertions alone overflow: refused in the normalisation itself
    out, exp = run(eng, [R.region(bytes(ref), cands, rlen=100)], R.options(), R.caps(cap_added=10), name="normalisation, cap_added")
    assert out["hdr"][0, 0] == 1 and out["hdr"][0, 5] == 6


# ---- c. sort, merge of equal variants, filter -----------------------------------------------------------------------------------------------------

def test_filter_of_the_golden_lists(eng, regionprep):
    cases = R.filter_cases(regionprep)
    groups = {}
    for reg, o, c, idx in cases:
        groups.setdefault((o["minReads"], o["maxSize"]), []).append(reg)
    assert sum(len(v) for v in groups.values()) == 60
    kept = 0
    for (mr, ms), regs in sorted(groups.items()):
        out, exp = run(eng, regs, R.options(minReads=mr, maxSize=ms), R.caps(cap_vars=128, cap_windows=128), name="filter, golden lists")
        kept += int(out["hdr"][:, 1].sum())
    assert kept == R.N_FILTER_KEPT


def test_sort_merge_and_filter_rules(eng):
    ref = bytearray(R.synth_ref(2000, 7))
    ref[400:420] = b"A" * 20
    ref[399:400], ref[420:421] = b"C", b"G"
    snp = lambda p: b"A" if ref[p:p + 1] != b"A" else b"C"
    cands = [(410, 1, b"", 3), (415, 1, b"", 4),                                 # one A of the run deleted at two places: one variant, 7 reads
             (100, 1, snp(100), 2), (110, 1, snp(110), 1),                       # support exactly minReads, and one below
             (600, 20, b"", 5), (700, 21, b"", 5),                               # size exactly maxSize, and one above (dropped)
             (1500, 30, b"", 5),                                                 # ... but the LAST run is kept: the reference has no size test there
             (50, 2, b"GT" if ref[50:52] != b"GT" else b"CA", 2), (50, 0, b"GG", 2), (50, 3, b"", 2), (50, 1, snp(50), 2),
             (50, 2, b"T" if ref[50:51] != b"T" else b"G", 2)]                   # all five types at one position, given out of order
    reg = R.region(bytes(ref), cands, rlen=100, reads=R.cover(1, 1900))
    out, exp = run(eng, [reg], R.options(minReads=2, maxSize=20), R.caps(), name="filter, rules")
    n = int(out["hdr"][0, 1])
    got = [(int(out["var_pos"][0, i]), int(out["var_nrem"][0, i]), int(out["var_nadd"][0, i]), int(out["var_support"][0, i])) for i in range(n)]
    assert got == [(50, 1, 1, 2), (50, 2, 2, 2), (50, 0, 2, 2), (50, 3, 0, 2), (50, 2, 1, 2), (100, 1, 1, 2), (399, 1, 0, 7), (600, 20, 0, 5), (1500, 30, 0, 5)]
    i = got.index((399, 1, 0, 7))
    assert (int(out["var_bam_min"][0, i]), int(out["var_bam_max"][0, i])) == (399, 420)
    # the oversized one in the middle goes, the same one as the last run stays; one read fewer on the last run and it goes too
    cands2 = [c for c in cands if c[0] != 1500] + [(1500, 30, b"", 1)]
    out, exp = run(eng, [R.region(bytes(ref), cands2, rlen=100)], R.options(minReads=2, maxSize=20), R.caps(), name="filter, rules")
    assert int(out["var_pos"][0, out["hdr"][0, 1] - 1]) == 600


def _thinned_region(n=200):
    """n SNPs three bases apart; the first ten and every third of the rest are seen in one read only (below minReads = 2)."""
    ref = R.synth_ref(1000, 19)
    cands = [(120 + 3 * i, 1, b"A" if ref[120 + 3 * i] != ord("A") else b"C", 1 if i < 10 or i % 3 == 0 else 2) for i in range(n)]
    return R.region(ref, cands, rlen=100), [int(c[3] >= 2) for c in cands]


def test_survivors_of_more_than_one_wave_with_gaps_in_the_first(eng):
    """The survivors are listed in order by a scan over the workgroup's threads, one sorted candidate a thread (wave_tiles.hpp,
    block_excl_scan): 200 candidates in four waves, the filter drops 28 of the first 64 and other counts of the later waves, so every
    wave's survivors start behind an offset that is not a multiple of 64."""
    reg, keep = _thinned_region()
    per_wave = [sum(keep[i:i + 64]) for i in range(0, 200, 64)]
    assert per_wave == [36, 43, 43, 5]
    out, exp = run(eng, [reg], R.options(minReads=2, maxVariants=8), R.caps(cap_vars=256, cap_windows=256), name="filter, survivors over waves")
    assert out["hdr"][0, :2].tolist() == [0, sum(keep)]
    assert out["var_pos"][0, :sum(keep)].tolist() == [120 + 3 * i for i in range(200) if keep[i]]


def test_equal_variants_from_different_placements_widen_the_bam_range(eng):
    """Two reads report one deletion at two places of a run LONGER than a normalisation window (rlen + 1 on either side): both walk to the
    run's left end, but the placement further left cannot see the run's right end and stops at its own window's end, so the two equal
    variants carry different bamMaxPos and Variant.addVariant has to widen the first one's.  (bamMinPos of equal variants is their common
    refPos: only the upper end can differ.)  The same for a deletion given at the run's left end below refPos 100, which is not
    normalised and carries [refPos, refPos], merged with one that is."""
    ref = _run_of(b"A", 150, at=600, total=1500, seed=43)
    low = _run_of(b"A", 30, at=85, total=900, seed=43)
    regions = [R.region(ref, [(620, 1, b"", 3), (690, 1, b"", 4)], rlen=100, reads=R.cover(1, 1400)),
               R.region(ref, [(690, 1, b"", 4, 0), (620, 1, b"", 3, 1)], rlen=100, reads=R.cover(1, 1400)),     # the wide one's record seen first
               R.region(ref, [(620, 1, b"", 3)], rlen=100, reads=R.cover(1, 1400)),
               R.region(low, [(84, 1, b"", 3), (105, 1, b"", 4)], rlen=100, reads=R.cover(1, 800))]
    out, exp = run(eng, regions, R.options(), R.caps(), name="filter, bam range widened")
    got = [[int(out[k][g, 0]) for k in ("var_pos", "var_support", "var_bam_min", "var_bam_max")] for g in range(4)]
    # 620 + 101 = 721 is where the left placement's window ends; the run ends at 750
    assert got == [[599, 7, 599, 750], [599, 7, 599, 750], [599, 3, 599, 721], [84, 7, 84, 115]] and out["hdr"][:, 1].tolist() == [1, 1, 1, 1]


def test_1024_candidates_are_taken_and_1025_are_not_and_cap_vars_and_cap_windows_fill_exactly(eng):
    ref = bytearray(R.synth_ref(3400, 9))
    cands = [(120 + 3 * i, 1, b"A" if ref[120 + 3 * i] != ord("A") else b"C", 2) for i in range(1025)]
    full = R.region(bytes(ref), cands[:1024], rlen=100)
    o = R.options(maxVariants=8)
    nw = len(R.expected_region(full, o, R.caps(cap_added=1024, cap_vars=1024, cap_windows=1024), 1025)["windows"])
    assert nw > 10
    for cp, status, reason in ((R.caps(cap_added=1024, cap_vars=1024, cap_windows=nw), 0, 0), (R.caps(cap_added=1024, cap_vars=1023, cap_windows=nw), 1, 6), (R.caps(cap_added=1024, cap_vars=1024, cap_windows=nw - 1), 1, 6)):
        out, exp = run(eng, [full], o, cp, cap_per_scan=1025, name="filter, SB_CAP and capacities")
        assert out["hdr"][0, [0, 5]].tolist() == [status, reason]
        if not status:
            assert out["hdr"][0, 1:3].tolist() == [1024, nw]
    over = R.region(bytes(ref), cands, rlen=100)
    out, exp = run(eng, [over, full], o, R.caps(cap_added=1024, cap_vars=1024, cap_windows=nw), cap_per_scan=1025, name="filter, SB_CAP and capacities")
    assert out["hdr"][:, [0, 5]].tolist() == [[1, 5], [0, 0]]
    # more candidates than cap_per_scan (what the merge reports with its own status), and the merge's status itself
    out, exp = run(eng, [R.region(bytes(ref), cands[:8], rlen=100, n_cands=9), R.region(bytes(ref), cands[:8], rlen=100, merge_status=R.ERR_OVERFLOW),
                         R.region(bytes(ref), cands[:8], rlen=100)], o, R.caps(), cap_per_scan=8, name="filter, SB_CAP and capacities")
    assert out["hdr"][:, [0, 5]].tolist() == [[1, 5], [1, 5], [0, 0]]


# ---- d. windows ------------------------------------------------------------------------------------------------------------------------------------

def test_windows_of_the_golden_regions(eng, regionprep):
    cases = R.window_cases(regionprep)
    groups = {}
    for k, (reg, o, c, idx) in enumerate(cases):
        groups.setdefault(tuple(sorted(o.items())), []).append(k)
    assert {(dict(g)["mergeClusteredVariants"], dict(g)["maxVariants"], dict(g)["largeWindows"]) for g in groups} >= {(0, 8, 0), (1, 3, 0), (1, 8, 1), (1, 8, 0)}
    assert {cases[k][0]["rlen"] for k in range(len(cases))} == {100, 150}
    n_in_place = n_windows = 0
    cp = R.caps(cap_vars=256, cap_windows=128, cap_added=4096, cap_batch_windows=2048, cap_batch_haps=1 << 15, cap_batch_reads=1 << 16, cap_hap_bytes=1 << 25)
    for g, ks in sorted(groups.items()):
        out, exp = run(eng, [cases[k][0] for k in ks], dict(g), cp, name="windows, golden")
        for j, k in enumerate(ks):
            reg, o, c, idx = cases[k]
            if not R.in_place(reg, exp["regions"][j]):
                continue
            # ... and the golden's own list, wherever the chain leaves the case's variants in place
            back = {i: m for m, i in enumerate(idx)}
            want = [[s, t, back[vs[0]], len(vs)] for s, t, vs in c["windows"] if vs and t - s <= o["maxSize"]]
            nw = int(out["hdr"][j, 2])
            got = [[int(out["win_start"][j, i]), int(out["win_end"][j, i]), int(out["win_var_first"][j, i]), int(out["win_var_n"][j, i])] for i in range(nw)]
            assert got == want, (k, got[:4], want[:4])
            n_in_place += 1
            n_windows += nw
    assert (len(cases), n_in_place, n_windows) == (R.N_WINDOW_CASES, R.N_WINDOW_CASES_IN_PLACE, R.N_WINDOWS_IN_PLACE)


def test_window_rules_at_their_edges(eng):
    ref = R.synth_ref(4000, 11)
    snp = lambda p, s=2: (p, 1, b"A" if ref[p:p + 1] != b"A" else b"C", s)
    reads = R.cover(1, 3900)
    # region [1000, 2000): variants at start - 1 (out), start, end - 1, end (out)
    r0 = R.region(ref, [snp(999), snp(1000), snp(1999), snp(2000)], start=1000, end=2000, rlen=100, reads=reads)
    # a window wider than maxSize is dropped (variantcaller.pyx:566-568): a deletion of 45 under maxSize 50
    r1 = R.region(ref, [snp(300), (500, 45, b"", 2), snp(800)], rlen=100, reads=reads)
    # gaps of minVarDist - 1, minVarDist, maxVarDist - 1, maxVarDist between neighbours, with maxVariants = 2 (the rule of the wide gap)
    ps = np.cumsum([1200, 8, 9, 14, 15, 8, 9, 14]).tolist()
    r2 = R.region(ref, [snp(p) for p in ps], rlen=100, reads=reads)
    # a deletion that reaches over the next variant, and one that ends just before it
    r3 = R.region(ref, [(2500, 30, b"", 2), snp(2520), (2700, 30, b"", 2), snp(2731), snp(2760)], rlen=100, reads=reads)
    o = R.options(maxSize=50, maxVariants=2)
    out, exp = run(eng, [r0, r1, r2, r3], o, R.caps(), name="windows, rules")
    assert [(int(out["win_start"][0, i]), int(out["win_end"][0, i])) for i in range(out["hdr"][0, 2])] == [(1000, 1009), (1990, 2008)]
    assert out["hdr"][1, 1:3].tolist() == [3, 2]
    assert [int(x) for x in out["win_var_n"][2, :out["hdr"][2, 2]]] == [w["n"] for w in exp["regions"][2]["windows"]]
    assert [(int(out["win_start"][2, i]), int(out["win_end"][2, i])) for i in range(out["hdr"][2, 2])] == [(1191, 1217), (1208, 1240), (1237, 1263), (1254, 1286)]
    assert out["win_var_n"][3, 0] == 2
    # the same under the other option sets
    for over in (dict(maxVariants=8), dict(mergeClusteredVariants=0), dict(largeWindows=1, maxSize=1500, maxVariants=3), dict(minVarDist=15, maxVarDist=9)):
        run(eng, [r0, r1, r2, r3], R.options(**dict(dict(maxSize=50, maxVariants=2), **over)), R.caps(), name="windows, rules")
    nw = [len(e["windows"]) for e in exp["regions"]]
    out, exp = run(eng, [r0, r1, r2, r3], o, R.caps(cap_windows=max(nw)), name="windows, rules")
    assert out["hdr"][:, 0].tolist() == [0, 0, 0, 0]
    out, exp = run(eng, [r0, r1, r2, r3], o, R.caps(cap_windows=max(nw) - 1), name="windows, rules")
    assert out["hdr"][:, [0, 5]].tolist() == [[int(n == max(nw)), 6 * int(n == max(nw))] for n in nw]


# ---- e. window pointers ----------------------------------------------------------------------------------------------------------------------------

def test_window_pointers_of_the_golden_read_arrays(eng, regionprep):
    cases = R.pointer_cases(regionprep)
    cp = R.caps(cap_vars=2, cap_windows=2, cap_added=8, cap_batch_windows=2048, cap_batch_haps=4096, cap_batch_reads=1 << 19, cap_hap_bytes=1 << 23)
    out, exp = run(eng, [c[0] for c in cases], R.options(**R.POINTER_OPTIONS), cp, name="window pointers, golden")
    n = 0
    for g, (reg, win, mwin, (s, t)) in enumerate(cases):
        assert out["hdr"][g, :3].tolist() == [0, 1, 1] and (int(out["win_start"][g, 0]), int(out["win_end"][g, 0])) == (s, t)
        assert out["win_ptrs"][g, 0].tolist() == win + win + mwin, (g, s, t)
        n += 1
    assert n == R.N_POINTER_QUERIES


def test_window_pointers_of_odd_tables(eng):
    ref = R.synth_ref(3000, 13)
    snp = lambda p: (p, 1, b"A" if ref[p:p + 1] != b"A" else b"C", 2)
    ending = [(p, 1491, 1491 - p) for p in range(1391, 1491, 9)]                 # every read ends at win_start exactly: none overlaps
    regions = [R.region(ref, [snp(1500)], rlen=100, reads=R.cover(1300, 1600), bad=[], broken=[]),                     # empty tables
               R.region(ref, [snp(1500)], rlen=100, reads=ending, bad=ending + [(1491, 1591, 100)], broken=[(10, 110, 100, 1495), (20, 120, 100, 1520)]),
               R.region(ref, [snp(60)], rlen=100, reads=R.cover(1, 400, 7), bad=R.cover(1, 400, 11), longest=[5000, 100, 0]),   # tab_longest > win_start
               R.region(ref, [snp(1500)], rlen=100, reads=[], bad=R.cover(1300, 1600))]                                # no good reads: skipped
    out, exp = run(eng, regions, R.options(), R.caps(), name="window pointers, odd tables")
    assert out["win_ptrs"][0, 0, 2:].tolist() == [0, 0, 0, 0]
    assert out["win_ptrs"][1, 0].tolist() == [len(ending), len(ending), len(ending), len(ending) + 1, 0, 1] and out["win_flags"][1, 0] == R.SBW_SKIP
    assert out["win_ptrs"][2, 0, 0] == 0 and out["win_flags"][3, 0] == R.SBW_SKIP


# ---- f. haplotypes ---------------------------------------------------------------------------------------------------------------------------------

def test_enumeration_and_validity_of_the_golden_sets(eng, golden_dir):
    cases = R.valid_cases(json.load(gzip.open(os.path.join(golden_dir, "filter_cases.json.gz"), "rt"))["valid"])
    cp = R.caps(cap_batch_windows=512, cap_batch_haps=8192, cap_batch_reads=8192, cap_hap_bytes=1 << 23)
    out, exp = run(eng, [reg for reg, _ in cases], R.options(**R.VALID_OPTIONS), cp, name="haplotypes, golden validity")
    n = 0
    for g, (reg, c) in enumerate(cases):
        if not R.in_place(reg, exp["regions"][g]):
            continue
        assert out["hdr"][g, :3].tolist() == [0, len(c["variants"]), 1] and out["win_flags"][g, 0] == 0
        bw = int(out["win_batch"][g, 0])
        masks = out["b_hap_mask"][out["b_hap_begin"][bw]:out["b_hap_begin"][bw + 1]].tolist()
        vs = [H.Variant("20", p, r.encode(), a.encode()) for p, r, a in c["variants"]]
        want = {0} | {sum(1 << i for i in x) for m in range(1, len(vs) + 1) for x in combinations(range(len(vs)), m) if H.isHaplotypeValid(tuple(vs[i] for i in x))}
        assert set(masks) == want and len(masks) == len(want) == out["win_n_haps"][g, 0]
        assert (((1 << len(vs)) - 1) in masks) == c["valid"], c
        n += 1
    assert (len(cases), n) == (R.N_VALID, R.N_VALID_IN_PLACE)


def test_haplotype_bytes_of_the_golden_cases(eng, golden_dir):
    cases = R.hapseq_cases(json.load(gzip.open(os.path.join(golden_dir, "hapseq_cases.json.gz"), "rt")))
    assert len(cases) == R.N_HAPSEQ and {c["rlen"] for _, _, c in cases} >= {36, 100, 150, 250, 400}
    groups = {}
    for k, (reg, o, c) in enumerate(cases):
        groups.setdefault(o["minVarDist"], []).append(k)
    cp = R.caps(cap_added=1024, cap_batch_windows=256, cap_batch_haps=4096, cap_batch_reads=1024, cap_hap_bytes=1 << 23)
    golden = 0
    for mvd, ks in sorted(groups.items()):
        out, exp = run(eng, [cases[k][0] for k in ks], cases[ks[0]][1], cp, name="haplotypes, golden bytes")
        for j, k in enumerate(ks):
            reg, o, c = cases[k]
            e = exp["regions"][j]
            full = (1 << len(c["variants"])) - 1
            if not R.in_place(reg, e) or len(e["windows"]) != 1 or e["windows"][0]["n"] != len(c["variants"]) or full not in e["windows"][0]["masks"]:
                continue
            if (e["windows"][0]["hap_start"], e["windows"][0]["hap_end"]) != (c["start_pos"], c["end_pos"]):
                continue
            bw = int(out["win_batch"][j, 0])
            h0, h1 = int(out["b_hap_begin"][bw]), int(out["b_hap_begin"][bw + 1])
            h = h0 + out["b_hap_mask"][h0:h1].tolist().index(full)
            assert out["b_hap_seq"][out["b_hap_off"][h]:out["b_hap_off"][h + 1]].tobytes() == c["haplotype"].encode(), k
            assert out["b_hap_off"][h + 1] - out["b_hap_off"][h] == len(c["haplotype"])
            assert (int(out["b_start"][bw]), int(out["b_end"][bw]), int(out["b_flank"][bw])) == (c["start_pos"], c["end_pos"], c["end_buffer"])
            golden += 1
    assert golden == R.N_HAPSEQ_GOLDEN_BYTES


def test_equal_haplotypes_merge_by_prior_or_go_to_the_caller(eng):
    ref = bytearray(R.synth_ref(1200, 17))
    ref[300:303] = b"TAC"
    ref[500:503] = b"TAC"
    ref[700:703] = b"TAC"
    ref[60:66] = b"GAAAAC"
    reads = R.cover(1, 1100, 30, 36)
    regions = [
        # MNP AC->GT against the SNPs A->G and C->T: one sequence; the MNP's prior is the better one (and it comes first)
        R.region(bytes(ref), [(301, 1, b"G", 2), (301, 2, b"GT", 2), (302, 1, b"T", 2)], rlen=36, reads=reads),
        # MNP TA->TG (one difference: 4.5e-5) against the SNP A->G (3.3e-4): the LATER haplotype has the better prior
        R.region(bytes(ref), [(500, 2, b"TG", 2), (501, 1, b"G", 2)], rlen=36, reads=reads),
        # MNP TA->TG against MNP AC->GC: one sequence, one prior: the first stays
        R.region(bytes(ref), [(700, 2, b"TG", 2), (701, 2, b"GC", 2)], rlen=36, reads=reads),
        # one A of a run deleted at two places below refPos 100 (not normalised): equal sequences with an indel among them
        R.region(bytes(ref), [(61, 1, b"", 2), (62, 1, b"", 2)], rlen=36, reads=reads),
        # a SNP that spells the reference: one haplotype is left, the loop does not call the window
        R.region(bytes(ref), [(900, 1, bytes(ref[900:901]), 2)], rlen=36, reads=reads)]
    out, exp = run(eng, regions, R.options(), R.caps(), name="haplotypes, equal sequences")
    assert out["win_flags"][:, 0].tolist() == [0, 0, 0, R.SBW_DUPLICATE, R.SBW_SKIP]
    masks = lambda g: out["b_hap_mask"][out["b_hap_begin"][out["win_batch"][g, 0]]:out["b_hap_begin"][out["win_batch"][g, 0] + 1]].tolist()
    assert sorted(masks(0)) == [0, 1, 2, 4] and sorted(masks(1)) == [0, 2] and sorted(masks(2)) == [0, 1] and sorted(masks(3)) == [0, 1, 2, 3]
    assert out["win_n_haps"][:, 0].tolist() == [4, 2, 2, 4, 0] and out["win_batch"][4, 0] == -1


def _boundary_regions():
    """Two haplotypes whose first difference lies d bytes behind the common prefix (a second SNP d bases behind the window's first variant),
    and a haplotype that is a strict prefix of another with d bytes behind the common prefix (a replacement that takes the contig's last
    bases away), for d = SB_STAGE - 1, SB_STAGE, SB_STAGE + 1."""
    regions = []
    for d in (R.SB_STAGE - 1, R.SB_STAGE, R.SB_STAGE + 1):
        ref = R.synth_ref(1400, 19)
        snp = lambda p: (p, 1, b"A" if ref[p:p + 1] != b"A" else b"C", 2)
        regions.append(R.region(ref, [snp(200), snp(200 + d)], rlen=100, reads=R.cover(1, 1300)))
        clen = 200 + d + 22
        tail = R.region(ref[:clen], [snp(200), (200 + d - 1, clen - 1 - (200 + d - 1), ref[200 + d - 1:200 + d], 2)], rlen=100, reads=R.cover(1, clen))
        regions.append(tail)
    return regions


def test_the_stage_of_384_bytes_decides_or_leaves_the_window_to_the_caller(eng):
    regions = _boundary_regions()
    o = R.options(largeWindows=1, maxVarDist=1000, maxSize=1500)
    out, exp = run(eng, regions, o, R.caps(), name="haplotypes, stage boundary")
    assert out["hdr"][:, :3].tolist() == [[0, 2, 1]] * 6
    assert out["win_flags"][:, 0].tolist() == [0, 0, R.SBW_DUPLICATE, R.SBW_DUPLICATE, R.SBW_DUPLICATE, R.SBW_DUPLICATE]
    assert out["win_n_haps"][:, 0].tolist() == [4] * 6


def test_width_of_the_enumeration_and_the_log2_threshold(eng):
    ref = R.synth_ref(3000, 23)
    snp = lambda p: (p, 1, b"A" if ref[p:p + 1] != b"A" else b"C", 2)
    cands = [snp(300 + 200 * n + 12 * i) for n in range(1, 7) for i in range(n)]        # windows of 1, 2, ... 6 variants
    reg = R.region(ref, cands, rlen=100, reads=R.cover(1, 2900))
    cp = R.caps(cap_batch_haps=128)
    want = {50: [0, 0, 0, 0, 0, 2], 33: [0, 0, 0, 0, 0, 2], 17: [0, 0, 0, 0, 2, 2], 3: [0, 2, 2, 2, 2, 2]}
    for mh, flags in want.items():
        out, exp = run(eng, [reg], R.options(maxHaplotypes=mh, filterVarsByCoverage=0), cp, name="haplotypes, width")
        assert out["win_var_n"][0, :6].tolist() == [1, 2, 3, 4, 5, 6] and out["win_flags"][0, :6].tolist() == flags
        assert out["win_n_haps"][0, :6].tolist() == [0 if f else 1 << (n + 1) for n, f in enumerate(flags)]
    # more variants than maxVariants in one window (neighbours closer than minVarDist are never split): skipped, or the caller's
    tight = R.region(ref, [snp(300 + 8 * i) for i in range(6)] + [snp(600 + 8 * i) for i in range(4)], rlen=100, reads=R.cover(1, 2900))
    for skip, flag in ((1, R.SBW_SKIP), (0, R.SBW_HOST)):
        out, exp = run(eng, [tight], R.options(maxHaplotypes=50, maxVariants=4, skipDifficultWindows=skip), cp, name="haplotypes, width")
        assert out["win_var_n"][0, :2].tolist() == [6, 4] and out["win_flags"][0, :2].tolist() == [flag, 0] and out["win_n_haps"][0, :2].tolist() == [0, 16]
    for fv in (0, 1):                                                            # filterVarsByCoverage with maxVariants <= log2(maxHaplotypes - 1)
        out, exp = run(eng, [reg, tight], R.options(maxHaplotypes=9, filterVarsByCoverage=fv, maxVariants=3), cp, name="haplotypes, width")
        assert all(f == (0 if n <= 3 else R.SBW_HOST) for f, n in zip(out["win_flags"][0, :out["hdr"][0, 2]].tolist(), out["win_var_n"][0].tolist()))
    out, exp = run(eng, [reg], R.options(maxHaplotypes=50, maxReads=2.0), cp, name="haplotypes, width")                         # too many reads: skipped
    assert out["win_flags"][0, :6].tolist() == [1] * 6


# ---- g. the batch as a whole -----------------------------------------------------------------------------------------------------------------------

def _batch_regions():
    ref = bytearray(R.synth_ref(3000, 29))
    ref[1500:1512] = b"A" * 12
    ref[1499:1500], ref[1512:1513] = b"C", b"G"
    ref = bytes(ref)
    snp = lambda p, s=2: (p, 1, b"A" if ref[p:p + 1] != b"A" else b"C", s)
    good = [(p, p + 100 + (p % 7), 100 + (p % 5)) for p in range(200, 2600, 23)]
    bad = [(p, p + 80, 80) for p in range(210, 2600, 97)]
    broken = sorted([(p, p + 100, 100, p + 300 - (p % 211)) for p in range(100, 2400, 131)], key=lambda r: r[3])
    edge = R.region(ref[600:], [(700, 1, b"", 2)], rlen=150, ref_seq_start=600, contig_len=3000, start=600, end=900, reads=good[:9], bad=bad[:2])   # flagged
    empty = R.region(ref, [], rlen=100, reads=good, bad=bad, broken=broken)
    plain = R.region(ref, [snp(400), snp(409), (600, 0, b"GATTACA", 3), snp(1000, 1), (1505, 1, b"", 4), (1508, 1, b"", 2), snp(1530), (2000, 3, b"", 2), snp(2003),
                           snp(2300), snp(2310), snp(2320)], rlen=100, reads=good, bad=bad, broken=broken)
    return [edge, empty, plain, R.region(ref, [snp(1200), snp(1210)], rlen=120, reads=good[10:60], broken=broken[:5])]


def test_the_batch_as_a_whole(eng):
    regions = _batch_regions()
    o = R.options()
    out, exp = run(eng, regions, o, R.caps(), name="batch")
    assert out["hdr"][:, 0].tolist() == [1, 0, 0, 0] and out["hdr"][0, 5] == 1 and out["hdr"][1, 1:3].tolist() == [0, 0]
    tot = out["totals"].tolist()
    nw, nh, nr = tot[:3]
    assert nw >= 5 and nh > 12 and nr > 50 and tot[10] == 0
    # the prefix arrays against sums recomputed from the per-window outputs
    wins = [(g, k) for g in range(len(regions)) if out["hdr"][g, 0] == 0 for k in range(out["hdr"][g, 2]) if out["win_flags"][g, k] in (0, R.SBW_DUPLICATE)]
    assert [int(out["win_batch"][g, k]) for g, k in wins] == list(range(nw))
    n_haps = [int(out["win_n_haps"][g, k]) for g, k in wins]
    n_reads = [int(sum(out["win_ptrs"][g, k, 2 * a + 1] - out["win_ptrs"][g, k, 2 * a] for a in range(3))) for g, k in wins]
    cum = lambda xs: np.concatenate([[0], np.cumsum(xs)]).tolist()
    assert out["b_hap_begin"][:nw + 1].tolist() == cum(n_haps) and out["b_read_begin"][:nw + 1].tolist() == cum(n_reads) == out["b_seg_begin"][:nw + 1].tolist()
    assert out["b_pair_off"][:nw + 1].tolist() == cum([h * r for h, r in zip(n_haps, n_reads)])
    assert out["b_gl_off"][:nw + 1].tolist() == cum([h * (h + 1) // 2 for h in n_haps])
    assert tot[:5] == [nw, sum(n_haps), sum(n_reads), sum(h * r for h, r in zip(n_haps, n_reads)), sum(h * (h + 1) // 2 for h in n_haps)]
    lens = np.diff(out["b_hap_off"][:nh + 1])
    assert tot[5] == lens.sum() == out["b_hap_off"][nh] and tot[7] == lens.max() and tot[8] == max(n_reads) and tot[9] == max(n_haps)
    a = R.pack(regions)
    read_len = np.diff(a["tables"]["read_off"])
    assert out["b_read_off"][:nr + 1].tolist() == cum(read_len[out["b_read_src"][:nr]]) and tot[6] == out["b_read_off"][nr]
    for (g, k), bw in zip(wins, range(nw)):
        r0 = int(out["b_read_begin"][bw])
        want = [(a["tables"]["tab_begin"][3 * g + t] + i, t) for t in range(3) for i in range(out["win_ptrs"][g, k, 2 * t], out["win_ptrs"][g, k, 2 * t + 1])]
        assert list(zip(out["b_read_src"][r0:r0 + len(want)].tolist(), out["b_read_kind"][r0:r0 + len(want)].tolist())) == want
        assert out["b_n_good"][bw] == out["win_ptrs"][g, k, 1] - out["win_ptrs"][g, k, 0]
        assert (int(out["b_start"][bw]), int(out["b_end"][bw]), int(out["b_flank"][bw])) == (max(int(out["win_start"][g, k]), 0), min(int(out["win_end"][g, k]), 2999),
                                                                                             min(2 * regions[g]["rlen"], 500))
    # a second call with the same inputs: the same content
    out2, _ = run(eng, regions, o, R.caps(), name="batch")
    for k in out:
        if k not in ("var_add_off", "added"):
            assert (out[k] == out2[k]).all(), k
    # every batch capacity exactly full, and one under
    full = dict(cap_batch_windows=nw, cap_batch_haps=nh, cap_batch_reads=nr, cap_hap_bytes=tot[5])
    out3, _ = run(eng, regions, o, R.caps(**full), name="batch")
    assert out3["totals"][10] == 0 and (out3["b_hap_seq"] == out["b_hap_seq"][:tot[5]]).all()
    for k in full:
        out4, _ = run(eng, regions, o, R.caps(**dict(full, **{k: full[k] - 1})), name="batch")
        assert out4["totals"][10] != 0 and out4["totals"][:10].tolist() == tot[:10]


# ---- a. the merge ----------------------------------------------------------------------------------------------------------------------------------

def _flip(b):
    return {65: 67, 67: 71, 71: 84, 84: 65}[b]


def _merge_scans():
    """Scans built by hand.  Scan c - 1 (c = 1 .. 40): c reads at one position; site s (s = 1 .. c) carries a SNP in the first s of them --
    every (supporting, covering) pair with 1 <= s <= c <= 40.  Then: a scan whose coverage depends on scan_longest and read_end (a long
    read from far left that still covers; reads ending exactly at the site; a deletion seen once under full coverage); an empty scan;
    a scan of two reads; and one region read as two scans."""
    ref = R.synth_ref(1200, 31)
    L = 30 + 12 * 40
    regs = []
    for c in range(1, 41):
        reads = []
        for k in range(c):
            seq = bytearray(ref[100:100 + L])
            for s in range(k + 1, c + 1):                                        # read k shows the sites s > k
                seq[15 + 12 * (s - 1)] = _flip(seq[15 + 12 * (s - 1)])
            reads.append(dict(seq=bytes(seq), qual=b"\x28" * L, pos=100, flag=3, cigar=[(0, L)], end=100 + L))
        regs.append(dict(ref=ref, ref_seq_start=0, contig_len=len(ref), reads=reads))
    site = 600
    mk = lambda pos, n: dict(seq=ref[pos:pos + n], qual=b"\x28" * n, pos=pos, flag=3, cigar=[(0, n)], end=pos + n)
    reads = [mk(150, 500)]                                                       # covers the site from far left: found only through scan_longest
    reads += [mk(100 + k, site - 100 - k) for k in range(5)]                     # end == site exactly, in front of every covering read: not counted
    reads += [mk(420, site - 420)]                                               # ... and one behind a covering read: the reference's loop counts it
    for k in range(6):                                                           # six reads over the site, two show the SNP
        pos = 520 + 5 * k
        seq = bytearray(ref[pos:pos + 150])
        if k < 2:
            seq[site - pos] = _flip(seq[site - pos])
        reads.append(dict(seq=bytes(seq), qual=b"\x28" * 150, pos=pos, flag=3, cigar=[(0, 150)], end=pos + 150))
    dpos = 560                                                                   # one read with a one-base deletion at 640 (seen once: passes as an indel)
    reads.append(dict(seq=ref[dpos:dpos + 81] + ref[dpos + 82:dpos + 151], qual=b"\x28" * 150, pos=dpos, flag=3, cigar=[(0, 81), (2, 1), (0, 69)], end=dpos + 151))
    reads.sort(key=lambda r: r["pos"])
    regs.append(dict(ref=ref, ref_seq_start=0, contig_len=len(ref), reads=reads))
    regs.append(dict(ref=ref, ref_seq_start=0, contig_len=len(ref), reads=[]))   # an empty scan
    # two reads, the first shows a SNP at 370 and the second starts behind it (test_merge_capacity_and_refusals hands their ends over wrong)
    seq = bytearray(ref[300:450])
    seq[70] = _flip(seq[70])
    regs.append(dict(ref=ref, ref_seq_start=0, contig_len=len(ref), reads=[dict(seq=bytes(seq), qual=b"\x28" * 150, pos=300, flag=3, cigar=[(0, 150)], end=450),
                                                                           dict(seq=ref[400:550], qual=b"\x28" * 150, pos=400, flag=3, cigar=[(0, 150)], end=550)]))
    two = []
    for k in range(8):                                                           # one region read as two scans of four reads: the same SNP in both halves
        seq = bytearray(ref[300:450])
        if k in (0, 1, 5):
            seq[70] = _flip(seq[70])
        two.append(dict(seq=bytes(seq), qual=b"\x28" * 150, pos=300, flag=3, cigar=[(0, 150)], end=450))
    regs.append(dict(ref=ref, ref_seq_start=0, contig_len=len(ref), reads=two))
    begin = np.concatenate([[0], np.cumsum([len(g["reads"]) for g in regs])]).tolist()
    begin = begin[:-1] + [begin[-2] + 4, begin[-1]]
    return ref, regs, begin


def _merge_expected(regs, begin, rec, count, max_per_read, read_seq_of, min_var_freq):
    """addVariantToList + `computeVariantReadSupportFrac(v) >= minVarFreq or nAdded != nRemoved` per scan, from the scan's records: {(first
    record id, supporting reads, covering reads, pos, nrem, nadd)}."""
    reads = [r for g in regs for r in g["reads"]]
    out = []
    for g in range(len(begin) - 1):
        mine = reads[begin[g]:begin[g + 1]]
        ra = H.ReadArray([H.AlignedRead(r["seq"], r["qual"], r["pos"], end=r["end"]) for r in mine])
        tally = {}
        for r in range(begin[g], begin[g + 1]):
            for k in range(count[r]):
                pos, nrem, nadd, ro, ao = rec[r, k].tolist()
                key = (pos, nrem, nadd, read_seq_of(ao, nadd))
                tally.setdefault(key, [r * max_per_read + k, 0])[1] += 1
        want = set()
        for (pos, nrem, nadd, _), (rid, n) in tally.items():
            total = ra.countReadsCoveringRegion(pos, pos + 1)
            frac = 0.0 if total == 0 else float(n) / total
            if frac >= min_var_freq or nadd != nrem:
                want.add((rid, n, total, pos, nrem, nadd))
        out.append(want)
    return out


def _scan(eng, regs):
    """The scan whose records the merge reads.  The engine keeps the LAST scan's records only, so every test that merges the fixture's
    scan runs it first: no test depends on which one ran before it."""
    eng.candidates(regs, max_per_read=64, retry=False, keep_device=True)


@pytest.fixture(scope="module")
def merge_scan(eng):
    ref, regs, begin = _merge_scans()
    _scan(eng, regs)
    lc = eng.last_candidates
    assert (lc["status"] == 0).all() and lc["count"].max() == 40
    reads = [r for g in regs for r in g["reads"]]
    longest = [max([r["end"] - r["pos"] for r in reads[begin[g]:begin[g + 1]]], default=0) for g in range(len(begin) - 1)]
    return dict(regs=regs, begin=begin, reads=reads, longest=longest, rec=lc["rec"], count=lc["count"], blob=lc["read_seq"].tobytes())


@pytest.mark.parametrize("thr", [0.05, 0.1, 0.2, 1.0 / 3.0])
def test_merge_counts_supports_and_coverage_and_filters_as_python_divides(eng, merge_scan, thr):
    m = merge_scan
    _scan(eng, m["regs"])
    assert (eng.last_candidates["rec"] == m["rec"]).all() and (eng.last_candidates["count"] == m["count"]).all()
    sent = Engine.sentinel_of("i4")
    cap = 48
    cand, n = eng.candidates_merge(m["begin"], [r["end"] for r in m["reads"]], m["longest"], thr, cap)
    want = _merge_expected(m["regs"], m["begin"], m["rec"], m["count"], 64, lambda ao, k: m["blob"][ao:ao + k], thr)
    seen = set()
    for g in range(len(want)):
        assert n[g, 1] == 0 and n[g, 0] == len(want[g]), (g, n[g].tolist(), len(want[g]))
        rows = cand[g, :n[g, 0]]
        assert {tuple(r[:6].tolist()) for r in rows} == want[g], g
        for r in rows:                                                           # the record's own fields, as the scan wrote them
            assert r[3:8].tolist() == m["rec"][r[0] // 64, r[0] % 64].tolist()
        assert (cand[g, n[g, 0]:] == sent).all(), (g, "rows behind out_n keep the sentinel")
        seen |= {(int(r[1]), int(r[2])) for r in rows if r[4] == r[5]}
    for g in range(40):                                                          # scan c - 1: site s passes exactly when float(s) / c >= thr
        c = g + 1
        assert sorted(int(r[1]) for r in cand[g, :n[g, 0]]) == [s for s in range(1, c + 1) if float(s) / c >= thr], (c, thr)
    assert seen >= {(s, c) for c in range(1, 41) for s in range(1, c + 1) if float(s) / c >= thr}
    far = {tuple(r[1:6].tolist()) for r in cand[40, :n[40, 0]]}
    # 600 is covered by the long read from far left, six short reads, the deletion's read and (as the reference counts) the read that ends
    # there behind the long one: 9, not the 5 in front that end there; the deletion seen once passes at any threshold
    assert far == ({(1, 9, 640, 1, 0), (2, 9, 600, 1, 1)} if 2.0 / 9 >= thr else {(1, 9, 640, 1, 0)})
    assert n[41].tolist() == [0, 0]                                              # the empty scan
    assert {tuple(r[1:4].tolist()) for r in cand[42, :n[42, 0]]} == {(1, 1, 370)}
    assert {tuple(r[1:4].tolist()) for r in cand[43, :n[43, 0]]} == {(2, 4, 370)} and {tuple(r[1:4].tolist()) for r in cand[44, :n[44, 0]]} == ({(1, 4, 370)} if 0.25 >= thr else set())
    print("[stage-b kernels] merge, threshold %.4f: %s" % (thr, json.dumps(dict(scans=len(want), records=int(m["count"].sum()), candidates=int(n[:, 0].sum()),
                                                                              refused=int((n[:, 1] != 0).sum())))))
    assert cand[43, 0, 0] == m["begin"][43] * 64 and (n[44, 0] == 0 or cand[44, 0, 0] == (m["begin"][44] + 1) * 64)     # the id of the FIRST record


def test_merge_capacity_and_refusals(eng, merge_scan):
    m = merge_scan
    _scan(eng, m["regs"])
    sent = Engine.sentinel_of("i4")
    ends = [r["end"] for r in m["reads"]]
    cand, n = eng.candidates_merge(m["begin"], ends, m["longest"], 0.0, 40)      # scan 39 holds 40 candidates: exactly full
    assert n[39].tolist() == [40, 0] and (n[:, 1] == 0).all() and (cand[39, :, 0] != sent).all()
    cand, n = eng.candidates_merge(m["begin"], ends, m["longest"], 0.0, 39)      # ... and one over; scan 38 is exactly full now
    assert n[39, 1] == R.ERR_OVERFLOW and (np.delete(n[:, 1], 39) == 0).all() and n[38].tolist() == [39, 0]
    # reads whose ends lie before the site they show, up to one that starts behind it (read pointers out of order): the reference raises
    # "Read start pointer > read end pointer" -- hostapi.ReadArray, the pinned mirror, does so for these very reads
    bad = list(ends)
    k = m["begin"][42]
    bad[k], bad[k + 1] = 360, 350
    with pytest.raises(RuntimeError, match="Read start pointer"):
        H.ReadArray([H.AlignedRead(b"A", b"!", 300, end=360), H.AlignedRead(b"A", b"!", 400, end=350)]).countReadsCoveringRegion(370, 371)
    cand, n = eng.candidates_merge(m["begin"], bad, m["longest"], 0.05, 48)
    assert n[42, 1] == R.ERR_BAD_INPUT and (np.delete(n[:, 1], 42) == 0).all()
    # a read with more records than max_per_read: -(2^20 + n); a read outside its reference window: PLAT_ERR_BAD_INPUT
    ref = R.synth_ref(600, 37)
    seq = bytearray(ref[100:250])
    for p in range(20, 140, 20):
        seq[p] = _flip(seq[p])
    rd = lambda s, pos: dict(seq=bytes(s), qual=b"\x28" * len(s), pos=pos, flag=3, cigar=[(0, len(s))], end=pos + len(s))
    regs = [dict(ref=ref, ref_seq_start=0, contig_len=600, reads=[rd(seq, 100), rd(ref[120:270], 120)]),
            dict(ref=ref[:400], ref_seq_start=0, contig_len=600, reads=[rd(ref[300:450], 300)]),
            dict(ref=ref, ref_seq_start=0, contig_len=600, reads=[rd(seq, 100), rd(seq, 100)])]
    eng.candidates(regs, max_per_read=4, retry=False, keep_device=True)
    assert eng.last_candidates["status"].tolist()[2] == R.ERR_BAD_INPUT
    cand, n = eng.candidates_merge([0, 2, 3, 5], [250, 270, 450, 250, 250], [150, 150, 150], 0.05, 8)
    assert n[:, 1].tolist() == [-(1 << 20) - 6, R.ERR_BAD_INPUT, -(1 << 20) - 6]
    assert (cand == sent).all()
    eng.candidates(regs[::2], max_per_read=6, retry=False, keep_device=True)                       # scanned again with room: merged
    lc = eng.last_candidates
    cand, n = eng.candidates_merge([0, 2, 4], [250, 270, 250, 250], [150, 150], 0.05, 6)
    blob = lc["read_seq"].tobytes()
    want = _merge_expected(regs[::2], [0, 2, 4], lc["rec"], lc["count"], 6, lambda ao, k: blob[ao:ao + k], 0.05)
    assert n.tolist() == [[6, 0], [6, 0]] and [{tuple(r[:6].tolist()) for r in cand[g]} for g in range(2)] == want
    assert sorted(cand[1, :, 1].tolist()) == [2] * 6 and sorted(cand[0, :, 1].tolist()) == [1] * 6
    print("[stage-b kernels] merge, capacity and refusals: %s" % json.dumps(dict(calls=5, scans=[45, 45, 45, 3, 2], refused=[0, 1, 1, 3, 0])))


# ---- h. the dictionary replay at kernel level ------------------------------------------------------------------------------------------------------

def test_two_alleles_of_equal_support_are_ordered_by_the_replayed_dictionaries(eng):
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
                seq[p - pos] = alts[(k + j) % 2] if j < 3 else alts[0]           # three sites with two alleles in turn, one with a single allele
        reads.append(dict(seq=bytes(seq), qual=b"\x28" * 150, pos=pos, flag=3, cigar=[(0, 150)], end=pos + 150))
    regs = [dict(ref=ref, ref_seq_start=0, contig_len=len(ref), reads=reads)]
    eng.candidates(regs, max_per_read=16, retry=False, keep_device=True)
    lc = eng.last_candidates
    blob = lc["read_seq"].tobytes()
    cand, n = eng.candidates_merge([0, len(reads)], [r["end"] for r in reads], [150], 0.05, 32)
    assert n[0, 1] == 0 and n[0, 0] == 7
    rows = sorted(cand[0, :n[0, 0]].tolist())
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
    assert sum(d[3] is not None for d in distinct) == len(cands)
    good = [(r["pos"], r["end"], len(r["seq"])) for r in reads]
    reg = R.region(ref, cands, rlen=150, start=400, end=1000, reads=good)
    a = R.pack([reg])
    h = _py2_string_hash("20")
    gd = [dict(start=400, end=1000, rlen=150, name_hash=h - (1 << 64) if h >= 1 << 63 else h)]
    o, cp = R.options(), R.caps()
    out = eng.stage_b(gd, a["tables"], o, with_records=True, **cp)
    exp = R.expected([reg], o, cp, 32, exact_records=[distinct])
    assert exp["regions"][0]["replay"] == 1 and exp["regions"][0]["status"] == 0
    R.compare(out, exp, [reg], cp, Engine.sentinel_of)
    assert out["hdr"][0, 6] == 1 and out["hdr"][0, 1] == 7
    print("[stage-b kernels] replay: %s" % json.dumps(R.counts(exp)))
    # the same candidates without the scan's records: the order is the dictionary's, the region the caller's
    out = eng.stage_b(gd, a["tables"], o, with_records=False, **cp)
    exp = R.expected([reg], o, cp, 32)
    assert exp["regions"][0]["reason"] == 2
    R.compare(out, exp, [reg], cp, Engine.sentinel_of)
    assert out["hdr"][0, [0, 5]].tolist() == [1, 2]
    # ... and by hand-made rows (cand_rec = NULL) as well
    out, exp = run(eng, [reg], o, cp, name="replay refused without records")
    assert out["hdr"][0, [0, 5]].tolist() == [1, 2]
