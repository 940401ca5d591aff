"""The inputs of tests/test_gpu_stage_b_fuzz.py (tests/stage_b_cases.py) on the CPU, through the mirror alone (tests/stage_b_reference.py):
the conditions the inputs were written to reach -- without which the comparisons on the device would hold without saying anything -- and a
second, independent statement of three steps where the mirror and the kernels share a line of descent (the sort key, isHaplotypeValid, the
haplotype bytes), written here from the rules' text and compared with the mirror on the whole corpus.  The figures asserted are conditions
on the inputs, not measurements."""
import collections
import gzip
import json
import os
import sys
import time
from itertools import combinations

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stage_b_cases as C  # noqa: E402
import stage_b_reference as R  # noqa: E402


@pytest.fixture(scope="module")
def calls():
    return C.corpus() + list(C.ladder().values())


@pytest.fixture(scope="module")
def expectations(calls):
    t = time.time()
    out = [R.expected(c["regions"], c["o"], c["cp"]) for c in calls]
    print("[stage-b fuzz] the mirror on %d calls, %d regions: %.2f s" % (len(calls), sum(len(c["regions"]) for c in calls), time.time() - t))
    assert time.time() - t < 30
    return out


def pairs(calls, expectations):
    for c, e in zip(calls, expectations):
        for reg, r in zip(c["regions"], e["regions"]):
            yield c, reg, r


# ---- the second statement -------------------------------------------------------------------------------------------------------------------------

def valid(vs):
    """platypusutils.pyx:735-802 over (pos, nrem, added) sorted: a variant covers [pos, max(pos, pos + nrem - 1)]; two neighbours must not
    share a base, except a SNP / MNP that ends on the base an insertion or deletion is labelled with."""
    for (p0, r0, a0), (p1, r1, a1) in zip(vs, vs[1:]):
        last = max(p0, p0 + r0 - 1)
        if last > p1 or (last == p1 and not (r0 == len(a0) and r1 != len(a1))):
            return False
    return True


def spelled(ref, rss, vs, lo, hi):
    """contig[lo:hi] with the variants (pos, nrem, added) applied by slicing, from the right: a SNP / MNP / replacement takes the place of
    its removed bases, an insertion goes behind its position, a deletion takes the bases behind its position away."""
    s, shift = ref, 0
    for pos, nrem, added in sorted(vs, key=lambda v: (v[0], len(v[2]) == v[1]), reverse=True):
        at = pos - rss
        if nrem and added:
            s = s[:at] + added + s[at + nrem:]
        elif added:
            s = s[:at + 1] + added + s[at + 1:]
        else:
            s = s[:at + 1] + s[at + 1 + nrem:]
        shift += len(added) - nrem
    return s[lo - rss:hi - rss + shift]


def apart(vs):
    """No two of the variants touch one base: a deletion labelled p takes p + 1 .. p + nrem away, which isHaplotypeValid lets the next
    variant start on (getMutatedSequence then goes its own way: not a case for slicing)."""
    spans = [(p + 1, p + 1 + nrem) if not a else (p, p + nrem) for p, nrem, a in vs if nrem]
    return all(x[1] <= y[0] for x, y in zip(spans, spans[1:]))


def test_the_sort_key_is_position_type_and_removed_length_and_stable(calls):
    n = ties = 0
    for c in calls:
        for reg in c["regions"]:
            if not reg["cands"]:
                continue
            fasta = R.WindowFasta(reg["name"], reg["ref"], reg["ref_seq_start"], reg["contig_len"])
            got = [(v.refPos, v.nRemoved, v.added) for v in sorted(R._variants(reg, fasta))]
            want = [(max(x[0], 0), x[1], x[2]) for x in sorted(reg["cands"], key=C.key)]
            assert got == want
            n += len(got)
            ties += len(got) - len({C.key(x) for x in reg["cands"]})
    assert n > 5000 and ties >= 10                                               # equal keys occur: stability is exercised


def test_validity_and_haplotype_bytes_by_slicing_equal_the_mirror(calls, expectations):
    """Every haplotype the mirror hands over: its mask must be a valid combination by valid() above, its bytes the contig with the variants
    applied by slicing; a window the device decides holds every valid combination unless mergeHaplotypes dropped one of an equal sequence."""
    windows = haps = dropped = later = quirk = touching = 0
    for c, reg, r in pairs(calls, expectations):
        for w in r["windows"]:
            if w["flags"] not in (0, R.SBW_DUPLICATE):
                continue
            vs = [(v["pos"], v["nrem"], v["added"]) for v in r["variants"][w["first"]:w["first"] + w["n"]]]
            lo = max(w["hap_start"] - w["end_buf"], 0)
            hi = min(w["hap_end"] + w["end_buf"], reg["contig_len"] - 1)
            masks = [sum(1 << i for i in x) for m in range(1, len(vs) + 1) for x in combinations(range(len(vs)), m) if valid([vs[i] for i in x])]
            assert set(w["masks"]) <= set([0] + masks), (c["name"], w)
            if w["flags"] == R.SBW_DUPLICATE:
                assert w["masks"] == [0] + masks
            inside = all(p >= w["hap_start"] and p + nrem + (0 if a else 1) <= w["hap_end"] for p, nrem, a in vs)
            if not inside:                                                        # (a variant that reaches the window's end: getMutatedSequence's own rule)
                quirk += 1
                continue
            pick = lambda m: [vs[i] for i in range(len(vs)) if m >> i & 1]
            seq = {m: spelled(reg["ref"], reg["ref_seq_start"], pick(m), lo, hi) for m in [0] + masks if apart(pick(m))}
            for m, s in zip(w["masks"], w["seqs"]):
                if m in seq:
                    assert s == seq[m], (c["name"], w["start"], m)
                    haps += 1
                else:
                    touching += 1
            windows += 1
            if w["flags"] == 0 and len(seq) == len(masks) + 1:
                assert sorted(set(seq.values())) == list(w["seqs"]), (c["name"], w["start"], "one haplotype per sequence, in sorted order")
                gone = [m for m in [0] + masks if m not in w["masks"]]
                dropped += bool(gone)
                later += any(seq[m] == seq[k] and ([0] + masks).index(k) > ([0] + masks).index(m) for m in gone for k in w["masks"])
    print("[stage-b fuzz] second statement: %d windows, %d haplotypes by slicing, %d windows and %d haplotypes left out; mergeHaplotypes dropped in %d, the later stayed in %d" % (
        windows, haps, quirk, touching, dropped, later))
    assert windows > 2000 and quirk < 0.05 * windows and touching < 0.05 * haps
    assert dropped >= 10 and later >= 3


# ---- reach conditions ------------------------------------------------------------------------------------------------------------------------------

def test_the_corpus_reaches_what_it_is_meant_to_reach(calls, expectations):
    regs = list(pairs(calls, expectations))
    reasons = collections.Counter(r["reason"] for _, _, r in regs if r["status"])
    flags = collections.Counter(w["flags"] for _, _, r in regs for w in r["windows"])
    by_n = collections.Counter(w["n"] for _, _, r in regs for w in r["windows"] if w["batch"] >= 0)
    n_haps = collections.Counter(w["n_haps"] for _, _, r in regs for w in r["windows"] if w["batch"] >= 0)
    chain = collections.Counter()
    for _, _, r in regs:
        chain.update({k: v for k, v in r.get("chain", {}).items() if k != "longest_key_run"})
    print("[stage-b fuzz] corpus: %d regions, reasons %s, window flags %s, variants per batch window %s, chain %s" % (
        len(regs), dict(reasons), dict(flags), dict(sorted(by_n.items())), dict(chain)))
    assert sum(reasons.values()) <= 0.25 * len(regs)
    assert all(reasons[k] >= 3 for k in (1, 2, 5, 6)) and set(reasons) == {1, 2, 5, 6}
    assert chain["moved"] >= 300
    assert chain["merged"] >= 40 and chain["mixed"] >= 10
    assert flags[0] >= 0.6 * sum(flags.values()) and all(flags[f] >= 15 for f in (R.SBW_SKIP, R.SBW_HOST, R.SBW_DUPLICATE))
    assert all(by_n[k] >= 20 for k in range(1, 6)) and n_haps[32] >= 1
    assert max(by_n) <= R.SB_MAXCOMB


def test_every_listed_size_occurs(calls, expectations):
    regs = list(pairs(calls, expectations))
    n_cands = {len(reg["cands"]) for _, reg, _ in regs}
    assert {0, 1, 2, 63, 64, 65, 200} <= n_cands and any(1000 <= n <= 1024 for n in n_cands)
    lad = C.ladder()
    on_device = lambda c: [r for r in R.expected(c["regions"], c["o"], c["cp"])["regions"]]
    # the size ladder stays on the device (distinct sort keys), the dense random regions do not
    assert all(r["status"] == 0 for name in ("candidates", "indels", "windows") for r in on_device(lad[name]))
    indels = [sum(C.pure_indel(x) and x[0] >= 100 for x in reg["cands"]) for reg in lad["indels"]["regions"]]
    assert indels == [0, 1, 15, 16, 17, 33]
    assert [len(r["windows"]) for r in on_device(lad["windows"])] == [255, 256, 257, 370, 1, 0]
    runs = on_device(lad["runs"])
    assert [r["chain"]["longest_key_run"] for r in runs[:4]] == [1, 2, 3, 48] and [r["status"] for r in runs] == [0, 0, 0, 0, 1] and runs[4]["reason"] == 2
    assert [len(r["variants"]) for r in runs[:4]] == [1, 1, 1, 1] and runs[3]["variants"][0]["support"] == sum(2 + i % 3 for i in range(48))
    dense = [r for c, reg, r in regs if len(reg["cands"]) > len({C.key(x) for x in reg["cands"]}) + 5]
    assert dense and all(r["status"] == 1 and r["reason"] == 2 for r in dense)
    # window counts per region, reads per window, haplotype lengths, walks of the normalisation
    reads_in_window = [w["ptrs"][1] - w["ptrs"][0] for _, _, r in regs for w in r["windows"] if None not in w["ptrs"]]
    assert min(reads_in_window) == 0 and 1 in reads_in_window and max(reads_in_window) > 256 and any(64 < n <= 256 for n in reads_in_window)
    ends_at_start = sum(any(rd[1] == w["start"] for rd in reg["reads"]) for _, reg, r in regs for w in r["windows"])
    assert ends_at_start >= 20                                                    # reads that end exactly where a window starts: not in it
    assert sum(w["ptrs"][2] is None for _, _, r in regs for w in r["windows"]) >= 10          # a table the reference raises on
    lens = [len(s) for _, _, r in regs for w in r["windows"] for s in w["seqs"]]
    assert min(lens) < 200 and max(lens) > 1000
    assert {reg["rlen"] for _, reg, _ in regs} == set(C.RLENS)
    walks = [v["bam_max"] - v["pos"] for _, _, r in regs for v in r["variants"]]
    assert any(64 <= d < 128 for d in walks) and any(128 <= d for d in walks) and any(0 < d < 64 for d in walks)
    assert sum(reg["ref_seq_start"] > 0 and reg["ref_seq_start"] + len(reg["ref"]) < reg["contig_len"] for _, reg, _ in regs) > 0.8 * len(regs)
    assert any(b"N" in reg["ref"] for _, reg, _ in regs)
    assert {len(c["regions"]) for c in calls} >= {5, 6, 8} and C.draw(130, 1) and len(C.all_regions()) > 130


# ---- the mirror against the reference's own texts on a subset of the corpus ---------------------------------------------------------------------

def test_the_mirror_equals_the_reference_on_the_wide_fixture(golden_dir, calls):
    """regionprep_wide_cases.json.gz (tests/golden/gen_golden.py: gen_regionprep_wide): 69 of the corpus' regions through the reference's
    leftNormaliseIndel, filterVariants, WindowGenerator, isHaplotypeValid and Haplotype texts.  The mirror's normalised list, kept list,
    windows and haplotype bytes must equal them wherever the mirror keeps the region (what it flags, it flags for the device's limits: the
    reference raised on none of these)."""
    cases = json.load(gzip.open(os.path.join(golden_dir, "regionprep_wide_cases.json.gz"), "rt"))
    n = dict(regions=0, flagged=0, normalised=0, with_range=0, kept=0, windows=0, haplotypes=0)
    for c in cases:
        g = calls[c["call"]]["regions"][c["region"]]
        assert (g["ref"].decode(), g["ref_seq_start"], g["contig_len"], g["start"], g["end"], g["rlen"]) == (c["ref"], c["ref_seq_start"], c["contig_len"], c["start"], c["end"], c["rlen"])
        assert [[x[0], x[1], x[2].decode(), x[3]] for x in g["cands"]] == c["cands"], "the generator no longer makes the fixture's regions"
        assert c["raised"] is None
        o = c["options"]
        lo, hi = min(x[0] for x in c["cands"]), max(x[0] for x in c["cands"])
        reg = dict(g, reads=R.cover(lo - 2 * g["rlen"], hi + 2 * g["rlen"], 10, g["rlen"]), bad=[], broken=[], longest=None)
        e = R.expected_region(reg, dict(o, maxReads=5000000.0), R.caps(cap_vars=1024, cap_windows=1024, cap_added=1 << 16), len(g["cands"]))
        n["regions"] += 1
        if e["status"]:
            assert e["reason"] in (1, 2), (c["call"], c["region"], e["reason"])
            n["flagged"] += 1
            continue
        want = [(p, r.encode(), a.encode(), lo_, hi_) for p, r, a, s, lo_, hi_ in c["normalised"]]
        assert e["normalised"] == want, (c["call"], c["region"])
        n["normalised"] += len(want)
        n["with_range"] += sum(v[3] != v[4] for v in want)
        got = [[v["pos"], v["removed"].decode(), v["added"].decode(), v["support"], v["bam_min"], v["bam_max"]] for v in e["variants"]]
        assert got == c["filtered"], (c["call"], c["region"])
        n["kept"] += len(got)
        wins = [w for w in c["windows"] if w[2] and w[1] - w[0] <= o["maxSize"]]
        assert [[w["start"], w["end"], list(range(w["first"], w["first"] + w["n"]))] for w in e["windows"]] == wins, (c["call"], c["region"])
        n["windows"] += len(wins)
        index = {tuple(w[:2]): i for i, w in enumerate(wins)}
        for wi, rows in c["haplotypes"]:
            assert isinstance(rows, list), rows
            w = e["windows"][index[tuple(c["windows"][wi][:2])]]
            if w["flags"] not in (0, R.SBW_DUPLICATE):
                continue
            ref_rows = {m: s.encode() for m, s in rows}
            assert all(ref_rows[m] == s for m, s in zip(w["masks"], w["seqs"])), (c["call"], c["region"], wi)
            if w["flags"] == R.SBW_DUPLICATE:
                assert w["masks"] == [m for m, _ in rows]                         # every valid combination, in itertools' order
            else:
                assert sorted(set(ref_rows.values())) == list(w["seqs"])
            n["haplotypes"] += len(w["masks"])
    print("[stage-b fuzz] wide fixture: %s" % json.dumps(n))
    assert n["regions"] == 69 and n["flagged"] <= 12 and n["with_range"] >= 150 and n["kept"] >= 800 and n["windows"] >= 300 and n["haplotypes"] >= 600
