"""The expected-value machinery of tests/test_gpu_stage_b_kernels.py (tests/stage_b_reference.py) against the committed goldens, on a
machine without a GPU: the module's chain must reproduce the `out` / `windows` / `window` / `mate_window` / `haplotype` / `valid` fields the
reference's own texts wrote, for the very regions the GPU tests hand to the kernels.  The counts asserted here were computed from the
fixtures when the tests were written; the GPU tests assert the same ones."""
import gzip
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stage_b_reference as R  # noqa: E402

@pytest.fixture(scope="module")
def regionprep(golden_dir):
    return json.load(gzip.open(os.path.join(golden_dir, "regionprep_cases.json.gz"), "rt"))


def test_normalisation_chain_reproduces_the_golden_out_and_predicts_the_flags(regionprep):
    cases = R.normalise_cases(regionprep)
    o, cp = R.options(**R.NORMALISE_OPTIONS), R.caps(**R.NORMALISE_CAPS)
    eligible = flagged = moved = 0
    for reg, v in cases:
        pos, nrem, added, _ = reg["cands"][0]
        assert reg["ref"][pos + 1:pos + 1 + nrem] == v["removed"].encode() if not added else reg["ref"][pos:pos + nrem] == v["removed"].encode()
        pure = nrem != len(added) and not (nrem and added) and pos >= 100
        eligible += pure
        e = R.expected_region(reg, o, cp, 1)
        if e["status"]:
            assert pure and e["reason"] == 1
            flagged += 1
            continue
        x = e["variants"][0]
        assert [x["pos"], x["removed"].decode(), x["added"].decode(), x["bam_min"], x["bam_max"], x["support"]] == v["out"][:6], (v, x)
        moved += x["pos"] != pos
    assert (len(cases), eligible, flagged) == (R.N_NORMALISE, R.N_NORMALISE_ELIGIBLE, R.N_NORMALISE_FLAGGED)
    assert flagged <= 0.01 * eligible                                             # what the device leaves to the caller stays rare
    assert moved + sum(v["out"][0] != v["pos"] for reg, v in cases if R.expected_region(reg, o, cp, 1)["status"]) == R.N_NORMALISE_MOVED


def test_filter_chain_equals_filterVariants_on_the_golden_lists(regionprep):
    """The lists restricted to the read-only candidates: the module's chain (sort, normalise, sort, filter) against the pinned
    filterVariants run directly on the restricted list, and against the golden rows that the restriction leaves untouched."""
    from types import SimpleNamespace
    from platypus_amd import hostapi as H
    lists = rows = golden_rows = flagged = 0
    for reg, o, c, idx in R.filter_cases(regionprep):
        e = R.expected_region(reg, o, R.caps(cap_vars=128), len(idx))
        lists += 1
        if e["status"]:
            assert e["reason"] == 2                                               # two alleles of one type at one position: the dictionary's order
            flagged += 1
            continue
        vs = [H.Variant("20", p, b"N" * n, a, s, H.PLATYPUS_VAR) for p, n, a, s in reg["cands"]]
        direct = H.filterVariants(list(vs), None, 150, c["min_reads"], c["max_size"], 0, SimpleNamespace(minReads=c["min_reads"], maxSize=c["max_size"]))
        unmoved = [v for v in e["variants"] if v["bam_min"] == v["bam_max"] == v["pos"]]
        got = {(v["pos"], v["nrem"], v["added"], v["support"]) for v in unmoved}
        assert got <= {(v.refPos, v.nRemoved, v.added, v.nSupportingReads) for v in direct}
        rows += len(e["variants"])
        # a golden row whose run holds read-only candidates alone (source 1) is a row of the restricted list too
        want = {(c["variants"][i]["pos"], len(c["variants"][i]["removed"]), c["variants"][i]["added"].encode(), n) for i, n, src, lo, hi in c["out"] if src == 1}
        golden_rows += len(want & got)
    assert lists == 60 and rows == R.N_FILTER_KEPT and rows > 300 and golden_rows > 100, (lists, rows, golden_rows, flagged)


def test_window_chain_reproduces_the_golden_windows(regionprep):
    cases = kept_cases = nwin = nwin_all = 0
    for reg, o, c, idx in R.window_cases(regionprep):
        e = R.expected_region(reg, o, R.caps(cap_vars=256, cap_windows=128, cap_added=4096), len(idx))
        cases += 1
        if not R.in_place(reg, e):
            continue
        kept_cases += 1
        back = {i: k for k, i in enumerate(idx)}
        want = [[s, t, [back[i] for i in vs]] for s, t, vs in c["windows"] if vs and t - s <= o["maxSize"]]
        got = [[w["start"], w["end"], list(range(w["first"], w["first"] + w["n"]))] for w in e["windows"]]
        assert got == want, (cases, got[:3], want[:3])
        nwin += len(got)
    assert (cases, kept_cases) == (R.N_WINDOW_CASES, R.N_WINDOW_CASES_IN_PLACE) and nwin == R.N_WINDOWS_IN_PLACE, (cases, kept_cases, nwin)


def test_window_pointers_reproduce_the_golden_windows_of_the_read_arrays(regionprep):
    n = exact = 0
    for reg, win, mwin, (s, t) in R.pointer_cases(regionprep):
        e = R.expected_region(reg, R.options(**R.POINTER_OPTIONS), R.caps(), 1)
        assert e["status"] == 0 and len(e["windows"]) == 1
        w = e["windows"][0]
        n += 1
        if (w["start"], w["end"]) == (s, t):
            assert w["ptrs"] == win + win + mwin, (s, t, w["ptrs"], win, mwin)
            exact += 1
    assert n == R.N_POINTER_QUERIES and exact == R.N_POINTER_QUERIES, (n, exact)


def test_enumeration_reproduces_the_golden_validity(golden_dir):
    cases = json.load(gzip.open(os.path.join(golden_dir, "filter_cases.json.gz"), "rt"))["valid"]
    n = kept = 0
    for reg, c in R.valid_cases(cases):
        n += 1
        e = R.expected_region(reg, R.options(**R.VALID_OPTIONS), R.caps(), len(reg["cands"]))
        if not R.in_place(reg, e):
            continue
        kept += 1
        assert len(e["windows"]) == 1 and e["windows"][0]["n"] == len(c["variants"]) and e["windows"][0]["flags"] in (0, R.SBW_DUPLICATE)
        full = (1 << len(c["variants"])) - 1
        assert (full in e["windows"][0]["masks"]) == c["valid"], c
    assert (n, kept) == (R.N_VALID, R.N_VALID_IN_PLACE), (n, kept)


def test_haplotype_bytes_reproduce_the_golden_haplotypes(golden_dir):
    cases = json.load(gzip.open(os.path.join(golden_dir, "hapseq_cases.json.gz"), "rt"))
    n = golden = 0
    for reg, o, c in R.hapseq_cases(cases):
        n += 1
        e = R.expected_region(reg, o, R.caps(cap_added=1024), len(reg["cands"]))
        if not R.in_place(reg, e) or len(e["windows"]) != 1:
            continue
        w = e["windows"][0]
        full = (1 << len(c["variants"])) - 1
        if w["n"] != len(c["variants"]) or (w["hap_start"], w["hap_end"]) != (c["start_pos"], c["end_pos"]) or full not in w["masks"]:
            continue
        assert w["seqs"][w["masks"].index(full)] == c["haplotype"].encode() and w["end_buf"] == c["end_buffer"]
        golden += 1
    assert (n, golden) == (R.N_HAPSEQ, R.N_HAPSEQ_GOLDEN_BYTES), (n, golden)
